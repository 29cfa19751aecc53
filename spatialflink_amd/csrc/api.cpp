// api.cpp -- C ABI of libgeoflink_hip.so (include/geoflink_hip.h): contexts, plans built once
// per continuous query (the reference computes its guaranteed / candidate cell sets once per
// operator, PointPointRangeQuery.java:119-125), and the per-window entry points.
#define GF_TU_NAME api_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "gf_internal.hpp"

using gf::AxisIv;
using gf::QueryRect;

// ---------------------------------------------------------------------------------------
// errors, context plumbing
// ---------------------------------------------------------------------------------------
namespace gf {

int set_err(gf_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->last_error = msg;
  return code;
}

int hip_err(gf_ctx* ctx, hipError_t e, const char* what) {
  char buf[512];
  snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  return set_err(ctx, e == hipErrorOutOfMemory ? GF_ERR_NOMEM : GF_ERR_HIP, buf);
}

int bind(gf_ctx* ctx) {
  hipError_t e = hipSetDevice(ctx->device);
  return e == hipSuccess ? GF_OK : hip_err(ctx, e, "hipSetDevice");
}

void* ctx_scratch(gf_ctx* ctx, size_t bytes, int* status) {
  *status = GF_OK;
  if (bytes <= ctx->scratch_bytes) return ctx->scratch;
  hipStreamSynchronize(ctx->stream);  // scratch may still be in use by queued work
  if (ctx->scratch) hipFree(ctx->scratch);
  ctx->scratch = nullptr;
  ctx->scratch_bytes = 0;
  size_t sz = std::max(bytes, (size_t)1 << 20);
  hipError_t e = hipMalloc(&ctx->scratch, sz);
  if (e != hipSuccess) { *status = hip_err(ctx, e, "hipMalloc(scratch)"); return nullptr; }
  ctx->scratch_bytes = sz;
  return ctx->scratch;
}

void* ctx_pinned(gf_ctx* ctx, size_t bytes, int* status) {
  *status = GF_OK;
  if (bytes <= ctx->pinned_bytes) return ctx->pinned;
  hipStreamSynchronize(ctx->stream);
  if (ctx->pinned) hipHostFree(ctx->pinned);
  ctx->pinned = nullptr;
  ctx->pinned_bytes = 0;
  size_t sz = std::max(bytes, (size_t)1 << 16);
  hipError_t e = hipHostMalloc(&ctx->pinned, sz, hipHostMallocDefault);
  if (e != hipSuccess) { *status = hip_err(ctx, e, "hipHostMalloc"); return nullptr; }
  ctx->pinned_bytes = sz;
  return ctx->pinned;
}

// One device scalar -> host through the pinned staging, then a stream sync (a pageable
// destination is copied by a staged blit, ~50 us per call in the join's rocprofv3 trace).
template <class T>
static int read_scalar_sync(gf_ctx* ctx, const void* dev, T* out) {
  int st = GF_OK;
  T* h = (T*)ctx_pinned(ctx, sizeof(T), &st);
  if (!h) return st;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(h, dev, sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  *out = *h;
  return GF_OK;
}

static hipEvent_t take_event(gf_ctx* ctx) {
  if (!ctx->pool.empty()) {
    hipEvent_t e = ctx->pool.back();
    ctx->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  hipEventCreate(&e);
  return e;
}

KTimer::KTimer(gf_ctx* c, int k) : ctx(c), kid(k) {
  if (!(ctx->timing & (1 << k))) return;
  if (ctx->timing_period > 1 && (ctx->timing_seq[k]++ % ctx->timing_period) != 0) return;
  a = take_event(ctx);
  b = take_event(ctx);
  hipEventRecord(a, ctx->stream);
}
KTimer::~KTimer() {
  if (!a) return;
  hipEventRecord(b, ctx->stream);
  ctx->pending.push_back({a, b, kid});
}

// Carve several aligned buffers out of one scratch allocation.
struct Arena {
  size_t off = 0;
  template <class T>
  size_t take(size_t count) {
    size_t o = (off + 255) & ~(size_t)255;
    off = o + count * sizeof(T);
    return o;
  }
};

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

static double first_at_least(int64_t A, double mn, double cl) {
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
static AxisIv axis_iv(int64_t a, int64_t b, double mn, double cl) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (a > b) return {nan, nan};
  AxisIv iv;
  iv.lo = first_at_least(a, mn, cl);
  iv.hi_excl = first_at_least(b + 1, mn, cl);
  return iv;
}

static QueryRect make_qrect(const gf_grid& g, int32_t qcx, int32_t qcy, int32_t gl, int32_t cl) {
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

static bool grid_ok(const gf_grid* g) {
  return g && g->n > 0 && std::isfinite(g->minX) && std::isfinite(g->minY) && std::isfinite(g->cellLength) &&
         g->cellLength > 0.0;
}

static int check_points(gf_ctx* ctx, const gf_points* p) {
  if (!p || p->n < 0) return set_err(ctx, GF_ERR_ARG, "invalid gf_points");
  if (p->n > (int64_t)UINT32_MAX) return set_err(ctx, GF_ERR_ARG, "window larger than 2^32-1 points");
  if (p->n > 0 && (!p->x || !p->y)) return set_err(ctx, GF_ERR_ARG, "null x/y");
  if ((((uintptr_t)p->x) | ((uintptr_t)p->y)) & 15) return set_err(ctx, GF_ERR_ALIGN, "x/y must be 16-byte aligned");
  return GF_OK;
}

static int stream_blocks(gf_ctx* ctx, int64_t items_per_thread_pairs) {
  int64_t b = (items_per_thread_pairs + kBlock - 1) / kBlock;
  const int64_t cap = (int64_t)ctx->num_cus * 8;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace gf

using namespace gf;


// ---------------------------------------------------------------------------------------
// library / context
// ---------------------------------------------------------------------------------------
extern "C" int gf_abi_version(void) { return GF_ABI_VERSION; }

namespace gf {  // one per translation unit (gf_buildtag.hpp)
const char* build_tag_api_cpp();
const char* build_tag_comm_cpp();
const char* build_tag_sliding_cpp();
const char* build_tag_csv_cpp();
const char* build_tag_objid_cpp();
const char* build_tag_k_points_hip();
const char* build_tag_k_knn_hip();
const char* build_tag_k_range_hip();
const char* build_tag_k_join_hip();
const char* build_tag_k_csv_hip();
const char* build_tag_k_objid_hip();
const char* build_tag_traj_cpp();
const char* build_tag_k_traj_hip();
struct UnitTag {
  const char* unit;
  const char* (*tag)();
};
static const UnitTag kUnitTags[] = {
    {"api.cpp", build_tag_api_cpp},         {"comm.cpp", build_tag_comm_cpp},
    {"sliding.cpp", build_tag_sliding_cpp}, {"csv.cpp", build_tag_csv_cpp},
    {"objid.cpp", build_tag_objid_cpp},     {"k_points.hip", build_tag_k_points_hip},
    {"k_knn.hip", build_tag_k_knn_hip},     {"k_range.hip", build_tag_k_range_hip},
    {"k_join.hip", build_tag_k_join_hip},   {"k_csv.hip", build_tag_k_csv_hip},
    {"k_objid.hip", build_tag_k_objid_hip}, {"traj.cpp", build_tag_traj_cpp},
    {"k_traj.hip", build_tag_k_traj_hip},
};
// run-time A/B knobs (valid alternative paths, never wrong results): reported, not refused
static const char* const kEnvKnobs[] = {"GF_K2_LSD", "GF_K2_SELFCOUNT", "GF_K2_ROWSORT", "GF_K2_MERGE", "GF_JOIN_BAND_PER_CU", "GF_JOIN_ROWPROBE",
                                        "GF_JOIN_CHUNK", "GF_RADIX_NT"};
}  // namespace gf

extern "C" int gf_build_is_product(void) {
  for (const auto& u : kUnitTags)
    if (u.tag()[0] != 0) return 0;
  return 1;
}

extern "C" const char* gf_build_info(void) {
  static std::string info = [] {
    std::string s = "gfx950 abi " + std::to_string(GF_ABI_VERSION) + "; defines:";
    bool any = false;
    for (const auto& u : kUnitTags)
      if (u.tag()[0]) {
        s += std::string(" [") + u.unit + ":" + u.tag() + "]";
        any = true;
      }
    if (!any) s += " none (product)";
    s += "; env:";
    bool anyenv = false;
    for (const char* k : kEnvKnobs)
      if (const char* v = std::getenv(k)) {
        s += std::string(" ") + k + "=" + v;
        anyenv = true;
      }
    if (!anyenv) s += " none";
    return s;
  }();
  return info.c_str();
}

extern "C" const char* gf_status_string(int s) {
  switch (s) {
    case GF_OK: return "ok";
    case GF_ERR_ARG: return "invalid argument";
    case GF_ERR_CAPACITY: return "output capacity too small";
    case GF_ERR_HIP: return "HIP runtime error";
    case GF_ERR_NOMEM: return "out of device memory";
    case GF_ERR_LAYERS: return "candidate layers <= 0 (reference: System.exit(1))";
    case GF_ERR_ALIGN: return "x/y not 16-byte aligned";
    case GF_ERR_COMM: return "RCCL error (see gf_comm_last_error)";
    default: return "unknown status";
  }
}

extern "C" int gf_device_count(int* n) {
  if (!n) return GF_ERR_ARG;
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  *n = (e == hipSuccess) ? c : 0;
  return e == hipSuccess ? GF_OK : GF_ERR_HIP;
}

extern "C" int gf_ctx_create(int device, gf_ctx** out) {
  if (!out) return GF_ERR_ARG;
  *out = nullptr;
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return GF_ERR_HIP;
  gf_ctx* ctx = new gf_ctx();
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess) { delete ctx; return GF_ERR_HIP; }
  if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return GF_ERR_HIP; }
  ctx->stream = ctx->own_stream;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
    ctx->num_cus = cus;
  *out = ctx;
  return GF_OK;
}

extern "C" void gf_ctx_destroy(gf_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  if (ctx->dict) gf_objid_dict_destroy(ctx->dict);
  if (ctx->expand_ticket) hipFree(ctx->expand_ticket);
  if (ctx->expand_status) hipFree(ctx->expand_status);
  if (ctx->join_gctr) hipFree(ctx->join_gctr);
  if (ctx->join_hint) hipHostFree(ctx->join_hint);
  if (ctx->csv_head) hipHostFree(ctx->csv_head);
  if (ctx->join_hist) hipFree(ctx->join_hist);
  if (ctx->join_ovf) hipFree(ctx->join_ovf);
  if (ctx->geojson_check) hipFree(ctx->geojson_check);
  for (auto& e : ctx->pending) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
  for (auto e : ctx->pool) hipEventDestroy(e);
  if (ctx->scratch) hipFree(ctx->scratch);
  if (ctx->pinned) hipHostFree(ctx->pinned);
  if (ctx->own_stream) hipStreamDestroy(ctx->own_stream);
  for (hipStream_t a : {ctx->aux, ctx->aux2})
    if (a) {
      hipStreamSynchronize(a);
      hipStreamDestroy(a);
    }
  delete ctx;
}

extern "C" int gf_ctx_set_stream(gf_ctx* ctx, void* s) {
  if (!ctx) return GF_ERR_ARG;
  ctx->stream = (hipStream_t)s;  // NULL is the HIP null stream (what torch's default stream is)
  return GF_OK;
}
extern "C" void* gf_ctx_stream(gf_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

extern "C" int gf_ctx_join(gf_ctx* ctx) {
  if (!ctx) return GF_ERR_ARG;
  if (!ctx->aux) return GF_OK;
  int st = bind(ctx);
  if (st) return st;
  for (hipStream_t a : {ctx->aux, ctx->aux2}) {
    if (!a) continue;
    hipEvent_t ev = take_event(ctx);
    GF_HIP_CHECK(ctx, hipEventRecord(ev, a));
    GF_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, ev, 0));
    ctx->pool.push_back(ev);
  }
  return GF_OK;
}

extern "C" int gf_ctx_fork(gf_ctx* ctx) {
  if (!ctx) return GF_ERR_ARG;
  if (!ctx->aux) return GF_OK;
  int st = bind(ctx);
  if (st) return st;
  hipEvent_t ev = take_event(ctx);
  GF_HIP_CHECK(ctx, hipEventRecord(ev, ctx->stream));
  for (hipStream_t a : {ctx->aux, ctx->aux2})
    if (a) GF_HIP_CHECK(ctx, hipStreamWaitEvent(a, ev, 0));
  ctx->pool.push_back(ev);
  return GF_OK;
}

namespace gf {
int sync_aux(gf_ctx* ctx) {
  for (hipStream_t a : {ctx->aux, ctx->aux2})
    if (a) GF_HIP_CHECK(ctx, hipStreamSynchronize(a));
  return GF_OK;
}
}  // namespace gf

extern "C" int gf_ctx_synchronize(gf_ctx* ctx) {
  if (!ctx) return GF_ERR_ARG;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return sync_aux(ctx);
}

extern "C" const char* gf_ctx_last_error(gf_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

extern "C" int gf_ctx_set_flag(gf_ctx* ctx, int flag, int value) {
  if (!ctx) return GF_ERR_ARG;
  if (flag == GF_FLAG_JOIN_LEGACY) { ctx->join_legacy = value != 0; return GF_OK; }
  if (flag == GF_FLAG_JOIN_COARSE) { ctx->join_coarse = value != 0; return GF_OK; }
  if (flag == GF_FLAG_GEOJSON_WALK) { ctx->geojson_walk = value != 0; return GF_OK; }
  if (flag == GF_FLAG_JOIN_STREAM) { ctx->join_stream = value != 0; return GF_OK; }
  if (flag == GF_FLAG_GEOJSON_WAVE) { ctx->geojson_wave = value != 0; return GF_OK; }
  if (flag == GF_FLAG_GEOJSON_CHECK) {
    if (value && !ctx->geojson_check) {
      GF_HIP_CHECK(ctx, hipMalloc(&ctx->geojson_check, 4 * sizeof(unsigned long long)));
      GF_HIP_CHECK(ctx, hipMemsetAsync(ctx->geojson_check, 0, 4 * sizeof(unsigned long long), ctx->stream));
    } else if (!value && ctx->geojson_check) {
      GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
      GF_HIP_CHECK(ctx, hipFree(ctx->geojson_check));
      ctx->geojson_check = nullptr;
    }
    return GF_OK;
  }
  return set_err(ctx, GF_ERR_ARG, "gf_ctx_set_flag: unknown flag");
}

extern "C" int gf_geojson_check_counts(gf_ctx* ctx, unsigned long long out[4]) {
  if (!ctx || !out) return GF_ERR_ARG;
  if (!ctx->geojson_check) return set_err(ctx, GF_ERR_ARG, "gf_geojson_check_counts: GF_FLAG_GEOJSON_CHECK is off");
  GF_HIP_CHECK(ctx, hipMemcpyAsync(out, ctx->geojson_check, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   ctx->stream));
  GF_HIP_CHECK(ctx, hipMemsetAsync(ctx->geojson_check, 0, 4 * sizeof(unsigned long long), ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return GF_OK;
}

extern "C" int gf_ctx_set_timing(gf_ctx* ctx, int mask) {
  if (!ctx) return GF_ERR_ARG;
  ctx->timing = mask;
  return GF_OK;
}

extern "C" int gf_ctx_set_timing_period(gf_ctx* ctx, int period) {
  if (!ctx || period < 1) return GF_ERR_ARG;
  ctx->timing_period = period;
  for (int64_t& v : ctx->timing_seq) v = 0;
  return GF_OK;
}

extern "C" int gf_ctx_timing(gf_ctx* ctx, int kid, double* total_ms, int64_t* launches) {
  if (!ctx || kid < 0 || kid >= GF_K_COUNT) return GF_ERR_ARG;
  int st = bind(ctx);
  if (st) return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (int e = sync_aux(ctx)) return e;
  for (auto& e : ctx->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      ctx->acc_ms[e.kid] += ms;
      ctx->acc_n[e.kid] += 1;
    }
    ctx->pool.push_back(e.a);
    ctx->pool.push_back(e.b);
  }
  ctx->pending.clear();
  if (total_ms) *total_ms = ctx->acc_ms[kid];
  if (launches) *launches = ctx->acc_n[kid];
  ctx->acc_ms[kid] = 0.0;
  ctx->acc_n[kid] = 0;
  return GF_OK;
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
  size_t o_k0 = ar.take<uint32_t>(n), o_k1 = ar.take<uint16_t>(n), o_v1 = ar.take<uint32_t>(n);
  size_t o_ma = ar.take<uint32_t>(matA), o_msa = ar.take<uint32_t>(matA + 1);
  size_t o_mb = ar.take<uint32_t>(matB), o_msb = ar.take<uint32_t>(matB + 1);
  size_t o_flag = ar.take<uint32_t>(1);
  int st = 0;
  char* base = (char*)ctx_scratch(ctx, ar.off, &st);
  if (st) return st;
  auto U32 = [&](size_t o) { return (uint32_t*)(base + o); };
  RadixArgs a{};
  a.tile = radix_tile();
  a.x = pts->x; a.y = pts->y; a.n = n;
  a.minX = g->minX; a.minY = g->minY; a.cl = g->cellLength; a.gn = g->n;
  a.bits = kRadixMaxBits; a.nblk = blocks; a.rowmode = 1;
  // (GF_K2_SELFCOUNT=1, A/B only: a one-segment row's scatter block counts its own columns instead
  // of the histogram kernel -- r06 A/B 0.2028 / 0.1997 vs 0.1988 / 0.1991 ms, profiles/r06_k2b_ab.jsonl)
  const char* sce = std::getenv("GF_K2_SELFCOUNT");
  const bool self_count = sce && *sce == '1';
  // r06: one-segment rows sorted whole, each by one block with its output staged in LDS
  // (radix_row_sort_kernel); GF_K2_ROWSORT=0 (A/B only) leaves them to the segment path
  const char* rse = std::getenv("GF_K2_ROWSORT");
  const bool rowsort = !(rse && *rse == '0') && !self_count && kRowSeg <= radix_row_sort_cap();
  a.multiseg = rowsort ? U32(o_flag) : nullptr;  // zeroed by pass A's histogram
  // pass A: row keys -> k0 with the histogram of rows, scan, stable scatter by row
  a.kout = U32(o_k0);
  a.shift = kRadixMaxBits;
  a.M = U32(o_ma);
  a.Ms = U32(o_msa);
  GF_HIP_CHECK(ctx, launch_radix(ctx, 0, a, blocks));
  ExpandState es;
  if ((st = lookback_state(ctx, scan1_blocks(matA), &es))) return st;
  GF_HIP_CHECK(ctx, launch_scan1(ctx->stream, U32(o_ma), matA, U32(o_msa), nullptr, 0, 0, es));
  ctx->expand_base += (unsigned long long)scan1_blocks(matA);
  a.kin = U32(o_k0);
  a.vin = nullptr;
  a.kout = nullptr;
  a.kout16 = (uint16_t*)(base + o_k1);  // the columns (u16): the row is the position's
  a.vout = U32(o_v1);
  GF_HIP_CHECK(ctx, launch_radix(ctx, 1, a, blocks));
  // pass B: per row segment column histograms (one-segment rows count their own columns in the
  // scatter), one scan, stable scatter by column (perm only)
  RadixArgs b = a;
  b.kin = nullptr;
  b.kin16 = (const uint16_t*)(base + o_k1);
  b.kout16 = nullptr;
  b.vin = U32(o_v1);
  b.kout = nullptr;
  b.vout = perm;
  b.shift = 0;
  b.seg = kRowSeg;
  b.MsA = U32(o_msa);
  b.nblkA = blocks;
  b.M = U32(o_mb);
  b.Ms = U32(o_msb);
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
    if ((st = lookback_state(ctx, scan1_blocks(matB), &es))) return st;
    GF_HIP_CHECK(ctx, launch_scan1(ctx->stream, U32(o_mb), matB, U32(o_msb), nullptr, 0, 0, es));
    ctx->expand_base += (unsigned long long)scan1_blocks(matB);
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
  // the scatter's tile buffers bound the blocks per CU (radix_threads), >= ~4 tiles per block
  const int64_t tiles = (n + radix_tile() - 1) / radix_tile();
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>(tiles / 4, 1), (int64_t)radix_max_blocks(ctx->num_cus));
  if (passes >= 2 && g->n + 1 <= kRadixMaxDigits && !std::getenv("GF_K2_LSD"))
    return bucket_rows(ctx, g, pts, perm, cell_start, blocks);
  const int64_t mat = ((int64_t)1 << pbits) * blocks;
  Arena ar;
  size_t o_k[2] = {ar.take<uint32_t>(n), ar.take<uint32_t>(n)};
  size_t o_v[2] = {ar.take<uint32_t>(n), ar.take<uint32_t>(n)};
  size_t o_k0 = ar.take<uint32_t>(n);  // pass 0's keys (stored by its histogram)
  size_t o_m = ar.take<uint32_t>(mat), o_ms = ar.take<uint32_t>(mat + 1);
  char* base = (char*)ctx_scratch(ctx, ar.off, &st);
  if (st) return st;
  auto U32 = [&](size_t o) { return (uint32_t*)(base + o); };
  RadixArgs a{};
  a.tile = radix_tile();
  a.x = pts->x; a.y = pts->y; a.n = n;
  a.minX = g->minX; a.minY = g->minY; a.cl = g->cellLength; a.gn = g->n;
  a.bits = pbits; a.nblk = blocks;
  uint32_t* k0 = U32(o_k0);
  for (int p = 0; p < passes; ++p) {
    a.kin = p == 0 ? nullptr : U32(o_k[(p - 1) & 1]);
    a.vin = p == 0 ? nullptr : U32(o_v[(p - 1) & 1]);
    a.kout = p == 0 ? k0 : U32(o_k[p & 1]);
    a.shift = p * pbits;
    a.M = U32(o_m);
    a.Ms = U32(o_ms);
    GF_HIP_CHECK(ctx, launch_radix(ctx, 0, a, blocks));  // pass 0: keys -> k0
    ExpandState es;
    if ((st = lookback_state(ctx, scan1_blocks(mat), &es))) return st;
    GF_HIP_CHECK(ctx, launch_scan1(ctx->stream, U32(o_m), mat, U32(o_ms), nullptr, 0, 0, es));
    ctx->expand_base += (unsigned long long)scan1_blocks(mat);
    if (p == 0) a.kin = k0;  // the scatter reads the stored keys, index = position
    a.kout = U32(o_k[p & 1]);
    a.vout = p == passes - 1 ? perm : U32(o_v[p & 1]);
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
  const int64_t tiles = (n + radix_tile() - 1) / radix_tile();
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>(tiles / 4, 1), (int64_t)radix_max_blocks(ctx->num_cus));
  const int64_t mat = ((int64_t)1 << bits) * blocks;
  Arena ar;
  size_t o_k0 = ar.take<uint32_t>(n), o_k = ar.take<uint32_t>(n);
  size_t o_m = ar.take<uint32_t>(mat), o_ms = ar.take<uint32_t>(mat + 1);
  char* base = (char*)ctx_scratch(ctx, ar.off, &st);
  if (st) return st;
  auto U32 = [&](size_t o) { return (uint32_t*)(base + o); };
  RadixArgs a{};
  a.tile = radix_tile();
  a.x = pts->x; a.y = pts->y; a.n = n;
  a.minX = g->minX; a.minY = g->minY; a.cl = g->cellLength; a.gn = g->n;
  a.bits = bits; a.nblk = blocks; a.shift = 0;
  a.nbands = nbands;
  for (int j = 0; j < nbands; ++j) a.band_lo[j] = band_lo[j];
  a.kin = nullptr; a.vin = nullptr; a.kout = U32(o_k0); a.M = U32(o_m); a.Ms = U32(o_ms);
  GF_HIP_CHECK(ctx, launch_radix(ctx, 0, a, blocks));  // band keys -> k0, histograms
  ExpandState es;
  if ((st = lookback_state(ctx, scan1_blocks(mat), &es))) return st;
  GF_HIP_CHECK(ctx, launch_scan1(ctx->stream, U32(o_m), mat, U32(o_ms), nullptr, 0, 0, es));
  ctx->expand_base += (unsigned long long)scan1_blocks(mat);
  a.kin = U32(o_k0); a.kout = U32(o_k); a.vout = perm;
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

// ---------------------------------------------------------------------------------------
// range plans
// ---------------------------------------------------------------------------------------
namespace {

struct Rect { int64_t x0, x1, y0, y1; };

template <class T>
int upload(gf_ctx* ctx, T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  if (src.empty()) return GF_OK;
  GF_HIP_CHECK(ctx, hipMalloc(dst, src.size() * sizeof(T)));
  GF_HIP_CHECK(ctx, hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return GF_OK;
}

void add_rect(std::vector<int32_t>& diff, int64_t n, Rect r) {
  r.x0 = std::max<int64_t>(r.x0, 0); r.y0 = std::max<int64_t>(r.y0, 0);
  r.x1 = std::min<int64_t>(r.x1, n - 1); r.y1 = std::min<int64_t>(r.y1, n - 1);
  if (r.x0 > r.x1 || r.y0 > r.y1) return;
  const int64_t W = n + 1;
  diff[r.y0 * W + r.x0] += 1;
  diff[r.y0 * W + r.x1 + 1] -= 1;
  diff[(r.y1 + 1) * W + r.x0] -= 1;
  diff[(r.y1 + 1) * W + r.x1 + 1] += 1;
}

void prefix2d(std::vector<int32_t>& d, int64_t n) {
  const int64_t W = n + 1;
  for (int64_t y = 0; y <= n; ++y)
    for (int64_t x = 1; x <= n; ++x) d[y * W + x] += d[y * W + x - 1];
  for (int64_t y = 1; y <= n; ++y)
    for (int64_t x = 0; x <= n; ++x) d[y * W + x] += d[(y - 1) * W + x];
}

Rect expand(Rect b, int64_t e) { return {b.x0 - e, b.x1 + e, b.y0 - e, b.y1 + e}; }

// Candidate cells covered by closed regions at distance 0 from each of their points (axis-
// aligned rectangle polygons; every bbox in approximate mode) become kInside (3) and are
// accepted untested.  A cell's exact coordinate range is the closed box
// [X_c, prev(X_{c+1})] x [Y_c, prev(Y_{c+1})] (X_c = first_at_least(c)).  Cells inside one
// region are marked directly; a cell the regions only partly overlap is split at the regions'
// edges into closed sub-boxes, and is covered iff every sub-box lies in some region -- so
// cells straddling the shared edge of two adjacent squares count too.
void mark_inside(gf_range_plan* P, std::vector<uint8_t>& table, const std::vector<std::array<double, 4>>& regs) {
  const gf_grid& g = P->grid;
  const int64_t n = g.n;
  std::vector<double> XT(n + 1), YT(n + 1);
  for (int64_t c = 0; c <= n; ++c) {
    XT[c] = first_at_least(c, g.minX, g.cellLength);
    YT[c] = first_at_least(c, g.minY, g.cellLength);
  }
  auto hi = [](const std::vector<double>& T, int64_t c) {  // largest double of cell c
    return std::isnan(T[c + 1]) ? INFINITY : std::nextafter(T[c + 1], -INFINITY);
  };
  // cells of [lo, hi] (overlapping: o0..o1; wholly inside: i0..i1)
  auto span = [&](const std::vector<double>& T, double lo, double up, double mn, int64_t& o0, int64_t& o1,
                  int64_t& i0, int64_t& i1) {
    o0 = std::max<int64_t>(cell_index(lo, mn, g.cellLength), 0);
    o1 = std::min<int64_t>(cell_index(up, mn, g.cellLength), n - 1);
    i0 = o0;
    i1 = o1;
    while (i0 <= i1 && !(T[i0] >= lo)) ++i0;
    while (i1 >= i0 && !(hi(T, i1) <= up)) --i1;
  };
  std::unordered_map<int64_t, std::vector<int32_t>> partial;
  for (size_t k = 0; k < regs.size(); ++k) {
    const auto& b = regs[k];
    int64_t ox0, ox1, ix0, ix1, oy0, oy1, iy0, iy1;
    span(XT, b[0], b[2], g.minX, ox0, ox1, ix0, ix1);
    span(YT, b[1], b[3], g.minY, oy0, oy1, iy0, iy1);
    for (int64_t y = oy0; y <= oy1; ++y)
      for (int64_t x = ox0; x <= ox1; ++x) {
        const int64_t cell = y * n + x;
        if (table[cell] != 1) continue;
        const bool in = x >= ix0 && x <= ix1 && y >= iy0 && y <= iy1;
        if (in) table[cell] = 3;
        else partial[cell].push_back((int32_t)k);
      }
  }
  for (auto& kv : partial) {
    const int64_t cell = kv.first;
    if (table[cell] != 1 || kv.second.size() < 2) continue;  // one partial region never covers
    const int64_t cx = cell % n, cy = cell / n;
    const double x0 = XT[cx], x1 = hi(XT, cx), y0 = YT[cy], y1 = hi(YT, cy);
    std::vector<double> xs{x0, x1}, ys{y0, y1};
    for (int32_t k : kv.second) {
      const auto& b = regs[k];
      if (b[0] > x0 && b[0] < x1) xs.push_back(b[0]);
      if (b[2] > x0 && b[2] < x1) xs.push_back(b[2]);
      if (b[1] > y0 && b[1] < y1) ys.push_back(b[1]);
      if (b[3] > y0 && b[3] < y1) ys.push_back(b[3]);
    }
    std::sort(xs.begin(), xs.end());
    xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    std::sort(ys.begin(), ys.end());
    ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
    bool covered = true;
    for (size_t i = 0; covered && i + 1 < xs.size(); ++i)
      for (size_t j = 0; covered && j + 1 < ys.size(); ++j) {
        bool any = false;
        for (int32_t k : kv.second) {
          const auto& b = regs[k];
          if (b[0] <= xs[i] && xs[i + 1] <= b[2] && b[1] <= ys[j] && ys[j + 1] <= b[3]) { any = true; break; }
        }
        covered = any;
      }
    if (covered) table[cell] = 3;
  }
}

// Cell classes and candidate lists for a set of query objects with base cell rects B_o
// (a query point's cell, or every cell under a polygon's bbox -- Polygon.java:62).
int build_table(gf_range_plan* P, const std::vector<Rect>& base, bool need_lists,
                const std::vector<std::array<double, 4>>* inside = nullptr, bool lists_all = false) {
  gf_ctx* ctx = P->ctx;
  const int64_t n = P->grid.n;
  const int32_t g = P->g_layers, c = P->c_layers;
  if (n * n > (int64_t)1 << 30 || n > 16384) return set_err(ctx, GF_ERR_ARG, "grid too large for a cell table");
  std::vector<int32_t> dG((n + 1) * (n + 1), 0), dC((n + 1) * (n + 1), 0);
  std::vector<int32_t> extra;
  for (const Rect& b : base) {
    if (g > 0) add_rect(dG, n, expand(b, g));
    else if (g == 0) {
      add_rect(dG, n, b);
      if (b.x0 < 0 || b.y0 < 0 || b.x1 >= n || b.y1 >= n) {  // out-of-grid guaranteed cells
        auto cl32 = [](int64_t v) { return (int32_t)std::min<int64_t>(std::max<int64_t>(v, INT32_MIN), INT32_MAX); };
        extra.push_back(cl32(b.x0)); extra.push_back(cl32(b.x1));
        extra.push_back(cl32(b.y0)); extra.push_back(cl32(b.y1));
      }
    }
    if (c > 0) add_rect(dC, n, expand(b, c));
  }
  prefix2d(dG, n);
  prefix2d(dC, n);
  std::vector<uint8_t> table(n * n);
  for (int64_t y = 0; y < n; ++y)
    for (int64_t x = 0; x < n; ++x) {
      const int64_t i = y * (n + 1) + x;
      table[y * n + x] = dG[i] > 0 ? 2 : (dC[i] > 0 ? 1 : 0);
    }
  if (inside && P->r >= 0.0)
    mark_inside(P, table, *inside);
  for (uint8_t v : table) P->cls_cells[v & 3]++;
  std::vector<uint32_t> rows(n);
  for (int64_t y = 0; y < n; ++y) {
    int64_t lo = n, hi = -1;
    for (int64_t x = 0; x < n; ++x)
      if (table[y * n + x]) { lo = std::min(lo, x); hi = std::max(hi, x); }
    rows[y] = hi < 0 ? 0xffffu : (uint32_t)lo | ((uint32_t)hi << 16);  // empty: lo 65535 > hi 0
  }
  std::vector<uint32_t> rowoff(n);
  std::vector<uint8_t> spans;
  for (int64_t y = 0; y < n; ++y) {
    rowoff[y] = (uint32_t)spans.size();
    const int64_t lo = rows[y] & 0xffffu, hi = rows[y] >> 16;
    for (int64_t x = lo; x <= hi; ++x) spans.push_back(table[y * n + x]);
  }
  P->span_bytes = (int64_t)spans.size();
  while (spans.size() % 4) spans.push_back(0);
  if (spans.empty()) spans.assign(4, 0);
  int st;
  if ((st = upload(ctx, &P->table, table)) || (st = upload(ctx, &P->rows, rows)) ||
      (st = upload(ctx, &P->rowoff, rowoff)) || (st = upload(ctx, &P->spans, spans)))
    return st;
  if (n <= 2048) {  // division-free cells in the scan (thresholds staged in LDS)
    std::vector<double> xt(n + 1), yt(n + 1);
    for (int64_t c = 0; c <= n; ++c) {
      xt[c] = first_at_least(c, P->grid.minX, P->grid.cellLength);
      yt[c] = first_at_least(c, P->grid.minY, P->grid.cellLength);
    }
    P->x_lo = xt[0]; P->x_hi = xt[n]; P->y_lo = yt[0]; P->y_hi = yt[n];
    int64_t clo = n, chi = -1;  // union of the row spans (columns holding any class)
    for (int64_t y = 0; y < n; ++y)
      if ((rows[y] & 0xffffu) <= (rows[y] >> 16)) {
        clo = std::min<int64_t>(clo, rows[y] & 0xffffu);
        chi = std::max<int64_t>(chi, rows[y] >> 16);
      }
    P->sx_lo = chi < 0 ? xt[n] : xt[clo];  // empty: sx_lo == sx_hi, every x fails
    P->sx_hi = chi < 0 ? xt[n] : xt[chi + 1];
    int64_t rlo = n, rhi = -1;  // rows holding any class
    for (int64_t y = 0; y < n; ++y)
      if ((rows[y] & 0xffffu) <= (rows[y] >> 16)) {
        rlo = std::min<int64_t>(rlo, y);
        rhi = std::max<int64_t>(rhi, y);
      }
    P->sy_lo = rhi < 0 ? yt[n] : yt[rlo];
    P->sy_hi = rhi < 0 ? yt[n] : yt[rhi + 1];
    P->span_frac = chi < 0 ? 0.0 : (double)(chi - clo + 1) * (double)(rhi - rlo + 1) / ((double)n * (double)n);
    if ((st = upload(ctx, &P->xt, xt)) || (st = upload(ctx, &P->yt, yt))) return st;
  }

  P->n_extra = (int32_t)(extra.size() / 4);
  if ((st = upload(ctx, &P->extra, extra))) return st;
  if (!need_lists) return GF_OK;
  // candidate lists over a (c + 2)-cell reach (superset of every object within r)
  const int64_t reach = (int64_t)std::max(c, 0) + 2;
  double area = 0;
  for (const Rect& b : base) {
    Rect r = expand(b, reach);
    r.x0 = std::max<int64_t>(r.x0, 0); r.y0 = std::max<int64_t>(r.y0, 0);
    r.x1 = std::min<int64_t>(r.x1, n - 1); r.y1 = std::min<int64_t>(r.y1, n - 1);
    if (r.x0 <= r.x1 && r.y0 <= r.y1) area += double(r.x1 - r.x0 + 1) * double(r.y1 - r.y0 + 1);
  }
  if (area > 6.4e7) return GF_OK;  // too large: every candidate-cell point tests every object
  std::vector<int32_t> off(n * n + 1, 0);
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<int32_t> cur;
    std::vector<int32_t> lst;
    if (pass == 1) {
      for (int64_t i = 0; i < n * n; ++i) off[i + 1] += off[i];
      cur.assign(off.begin(), off.end() - 1);
      lst.resize(off[n * n]);
    }
    for (size_t o = 0; o < base.size(); ++o) {
      Rect r = expand(base[o], reach);
      r.x0 = std::max<int64_t>(r.x0, 0); r.y0 = std::max<int64_t>(r.y0, 0);
      r.x1 = std::min<int64_t>(r.x1, n - 1); r.y1 = std::min<int64_t>(r.y1, n - 1);
      for (int64_t y = r.y0; y <= r.y1; ++y)
        for (int64_t x = r.x0; x <= r.x1; ++x) {
          const int64_t cell = y * n + x;
          if (lists_all ? table[cell] == 0 : (table[cell] != 1 && table[cell] != 3)) continue;
          if (pass == 0) off[cell + 1]++;
          else lst[cur[cell]++] = (int32_t)o;
        }
    }
    if (pass == 1) {
      if ((st = upload(ctx, &P->cand_off, off))) return st;
      if (lst.empty()) lst.push_back(0);
      if ((st = upload(ctx, &P->cand_list, lst))) return st;
    }
  }
  return GF_OK;
}

// row-span class tables up to this size are staged in LDS by every scan block
constexpr int64_t kSpanLdsBytes = 32768;

// scan blocks (<= 8 per CU) + deferred-test blocks (8 per CU) of per-block partial counts
int finish_plan(gf_range_plan* P) {
  // partials of <= kRangeMaxParts blocks (scan <= 8 per CU + deferred tests), then the ticket
  if (P->ctx->num_cus * 16 > gf::kRangeMaxParts) return set_err(P->ctx, GF_ERR_ARG, "too many CUs for the partials");
  GF_HIP_CHECK(P->ctx, hipMalloc(&P->partials, sizeof(uint64_t) * (gf::kRangeTicketSlot + 1)));
  GF_HIP_CHECK(P->ctx, hipMemset(P->partials + gf::kRangeTicketSlot, 0, sizeof(uint64_t)));
  GF_HIP_CHECK(P->ctx, hipMalloc(&P->queue_count, sizeof(uint32_t) * (size_t)P->ctx->num_cus * 8));
  return GF_OK;
}



}  // namespace

extern "C" void gf_range_plan_destroy(gf_range_plan* P) {
  if (!P) return;
  hipSetDevice(P->ctx->device);
  hipStreamSynchronize(P->ctx->stream);
  void* bufs[] = {P->table, P->extra, P->cand_off, P->cand_list, P->qx, P->qy, P->ring_off, P->vert_off,
                  P->vx, P->vy, P->bbox, P->ring_env, P->partials, P->queue, P->queue_count, P->queue_xy, P->rows, P->xt, P->yt,
                  P->rowoff, P->spans, P->brect, P->rect, P->jecnt, P->jecand, P->jbtot, P->jtotal,
                  P->batch_partials};
  for (void* b : bufs)
    if (b) hipFree(b);
  delete P;
}

extern "C" int gf_range_pp_plan_create(gf_ctx* ctx, const gf_grid* g, const double* qx, const double* qy,
                                       int32_t nq, double r, int approximate, int metric, gf_range_plan** out) {
  if (!ctx || !out || !grid_ok(g) || nq < 0 || (nq > 0 && (!qx || !qy)) || (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, "gf_range_pp_plan_create: bad argument");
  *out = nullptr;
  int st = bind(ctx);
  if (st) return st;
  gf_range_plan* P = new gf_range_plan();
  P->ctx = ctx;
  P->grid = *g;
  P->r = r;
  P->approx = approximate != 0;
  P->metric = metric;
  P->nq = nq;
  P->g_layers = guaranteed_layers(g->cellLength, r);
  P->c_layers = candidate_layers(g->cellLength, r);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (nq == 0) {  // nothing is ever guaranteed or candidate
    P->table_mode = 0;
    P->qr.cgx = P->qr.cgy = P->qr.gx = P->qr.gy = {nan, nan};
    P->qr.g_any = 0;
  } else if (nq == 1) {
    P->table_mode = 0;
    const int32_t qcx = cell_index(qx[0], g->minX, g->cellLength), qcy = cell_index(qy[0], g->minY, g->cellLength);
    P->qr = make_qrect(*g, qcx, qcy, P->g_layers, P->c_layers);
    P->qx0 = qx[0];
    P->qy0 = qy[0];
  } else {
    P->table_mode = 1;
    std::vector<Rect> base(nq);
    for (int32_t q = 0; q < nq; ++q) {
      const int64_t cx = cell_index(qx[q], g->minX, g->cellLength), cy = cell_index(qy[q], g->minY, g->cellLength);
      base[q] = {cx, cx, cy, cy};
    }
    if ((st = build_table(P, base, !P->approx))) { gf_range_plan_destroy(P); return st; }
    std::vector<double> vqx(qx, qx + nq), vqy(qy, qy + nq);
    if ((st = upload(ctx, &P->qx, vqx)) || (st = upload(ctx, &P->qy, vqy))) { gf_range_plan_destroy(P); return st; }
  }
  if ((st = finish_plan(P))) { gf_range_plan_destroy(P); return st; }
  *out = P;
  return GF_OK;
}

namespace {
// join != 0: a point-polygon join plan -- cell lists for every non-none cell (guaranteed ones
// too: the join tests every co-located pair), no inside-cell marking, per-polygon bbox cells.
int ppoly_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_polygons* polys, double r, int approximate, int metric,
                      int join, gf_range_plan** out) {
  if (!ctx || !out || !grid_ok(g) || !polys || polys->npoly < 0 || (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, join ? "gf_join_ppoly_plan_create: bad argument"
                                         : "gf_range_ppoly_plan_create: bad argument");
  *out = nullptr;
  int st = bind(ctx);
  if (st) return st;
  const int32_t np = polys->npoly;
  const int32_t nrings = np > 0 ? polys->ring_off[np] : 0;
  // validate rings: >= 4 vertices, closed (Polygon.createPolygon / JTS LinearRing)
  for (int32_t p = 0; p < np; ++p)
    if (polys->ring_off[p + 1] <= polys->ring_off[p]) return set_err(ctx, GF_ERR_ARG, "polygon without a shell");
  for (int32_t j = 0; j < nrings; ++j) {
    const int32_t v0 = polys->vert_off[j], v1 = polys->vert_off[j + 1];
    if (v1 - v0 < 4 || polys->vx[v0] != polys->vx[v1 - 1] || polys->vy[v0] != polys->vy[v1 - 1])
      return set_err(ctx, GF_ERR_ARG, "ring must be closed with >= 4 vertices");
  }
  gf_range_plan* P = new gf_range_plan();
  P->ctx = ctx;
  P->grid = *g;
  P->r = r;
  P->approx = approximate != 0;
  P->metric = metric;
  P->poly = 1;
  P->table_mode = 1;
  P->npoly = np;
  P->nq = np;
  P->g_layers = guaranteed_layers(g->cellLength, r);
  P->c_layers = candidate_layers(g->cellLength, r);
  std::vector<double> bbox(4 * (size_t)std::max(np, 1)), renv(4 * (size_t)std::max(nrings, 1));
  for (int32_t j = 0; j < nrings; ++j) {
    const int32_t v0 = polys->vert_off[j], v1 = polys->vert_off[j + 1];
    double mnx = polys->vx[v0], mxx = mnx, mny = polys->vy[v0], mxy = mny;
    for (int32_t v = v0 + 1; v < v1; ++v) {
      mnx = std::min(mnx, polys->vx[v]); mxx = std::max(mxx, polys->vx[v]);
      mny = std::min(mny, polys->vy[v]); mxy = std::max(mxy, polys->vy[v]);
    }
    renv[4 * j] = mnx; renv[4 * j + 1] = mxx; renv[4 * j + 2] = mny; renv[4 * j + 3] = mxy;
  }
  std::vector<Rect> base(np);
  for (int32_t p = 0; p < np; ++p) {
    const int32_t sh = polys->ring_off[p];  // shell envelope = Polygon.getEnvelopeInternal
    const double x1 = renv[4 * sh], x2 = renv[4 * sh + 1], y1 = renv[4 * sh + 2], y2 = renv[4 * sh + 3];
    bbox[4 * p] = x1; bbox[4 * p + 1] = y1; bbox[4 * p + 2] = x2; bbox[4 * p + 3] = y2;
    base[p] = {cell_index(x1, g->minX, g->cellLength), cell_index(x2, g->minX, g->cellLength),
               cell_index(y1, g->minY, g->cellLength), cell_index(y2, g->minY, g->cellLength)};
  }
  // regions at distance 0 from each of their points: approximate mode -> every bbox;
  // exact mode -> shells that are axis-aligned rectangles without holes
  std::vector<std::array<double, 4>> inside;
  std::vector<uint8_t> rectf((size_t)std::max(np, 1), 0);
  for (int32_t p = 0; p < np; ++p) {
    const double x1 = bbox[4 * p], y1 = bbox[4 * p + 1], x2 = bbox[4 * p + 2], y2 = bbox[4 * p + 3];
    if (!(x1 < x2 && y1 < y2)) continue;
    bool rect = false;
    if (polys->ring_off[p + 1] - polys->ring_off[p] == 1) {
      const int32_t v0 = polys->vert_off[polys->ring_off[p]], v1 = polys->vert_off[polys->ring_off[p] + 1];
      int corners = 0;
      rect = (v1 - v0 == 5);
      for (int32_t v = v0; rect && v < v1; ++v) {
        const double X = polys->vx[v], Y = polys->vy[v];
        rect = (X == x1 || X == x2) && (Y == y1 || Y == y2);
        if (rect && v > v0) rect = (X == polys->vx[v - 1]) != (Y == polys->vy[v - 1]);  // one axis moves
        if (rect && v < v1 - 1) corners |= 1 << ((X == x2) + 2 * (Y == y2));
      }
      rect = rect && corners == 15;
    }
    rectf[p] = rect;
    if (rect || P->approx) inside.push_back({x1, y1, x2, y2});
  }
  P->join = join;
  if ((st = build_table(P, base, true, join ? nullptr : &inside, join != 0))) { gf_range_plan_destroy(P); return st; }
  if (join) {
    std::vector<int32_t> br(4 * (size_t)std::max(np, 1), 0);
    auto cl32 = [](int64_t v) { return (int32_t)std::min<int64_t>(std::max<int64_t>(v, INT32_MIN), INT32_MAX); };
    for (int32_t p = 0; p < np; ++p) {
      br[4 * p] = cl32(base[p].x0); br[4 * p + 1] = cl32(base[p].x1);
      br[4 * p + 2] = cl32(base[p].y0); br[4 * p + 3] = cl32(base[p].y1);
    }
    if ((st = upload(ctx, &P->brect, br))) { gf_range_plan_destroy(P); return st; }
    GF_HIP_CHECK(ctx, hipMalloc(&P->jbtot, sizeof(uint32_t) * (size_t)ctx->num_cus * 8));
    GF_HIP_CHECK(ctx, hipMalloc(&P->jtotal, sizeof(unsigned long long)));
  }
  const int32_t nverts = nrings > 0 ? polys->vert_off[nrings] : 0;
  std::vector<int32_t> ro(polys->ring_off, polys->ring_off + np + 1), vo(polys->vert_off, polys->vert_off + nrings + 1);
  std::vector<double> vx(polys->vx, polys->vx + nverts), vy(polys->vy, polys->vy + nverts);
  if ((st = upload(ctx, &P->ring_off, ro)) || (st = upload(ctx, &P->vert_off, vo)) || (st = upload(ctx, &P->vx, vx)) ||
      (st = upload(ctx, &P->vy, vy)) || (st = upload(ctx, &P->bbox, bbox)) || (st = upload(ctx, &P->ring_env, renv)) ||
      (st = upload(ctx, &P->rect, rectf))) {
    gf_range_plan_destroy(P);
    return st;
  }
  if ((st = finish_plan(P))) { gf_range_plan_destroy(P); return st; }
  *out = P;
  return GF_OK;
}
}  // namespace

extern "C" int gf_range_ppoly_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_polygons* polys, double r,
                                          int approximate, int metric, gf_range_plan** out) {
  return ppoly_plan_create(ctx, g, polys, r, approximate, metric, 0, out);
}

extern "C" int gf_join_ppoly_plan_create(gf_ctx* ctx, const gf_grid* qgrid, const gf_polygons* polys, double r,
                                         int approximate, int metric, gf_range_plan** out) {
  return ppoly_plan_create(ctx, qgrid, polys, r, approximate, metric, 1, out);
}

namespace {
RangeArgs range_args(const gf_range_plan* P, const gf_points* pts, uint64_t* bitmap, uint64_t* multi) {
  RangeArgs a{};
  a.x = pts->x; a.y = pts->y; a.n = pts->n;
  a.bitmap = bitmap; a.multi = multi; a.partials = P->partials;
  a.nq = P->nq;
  a.qr = P->qr;
  a.grid_n = P->grid.n; a.minX = P->grid.minX; a.minY = P->grid.minY; a.cl = P->grid.cellLength;
  a.table = P->table; a.rows = P->rows; a.extra = P->extra; a.n_extra = P->n_extra;
  a.rowoff = P->rowoff; a.spans = P->spans; a.span_bytes = (int32_t)std::min<int64_t>(P->span_bytes, INT32_MAX);
  a.span_lds = P->span_bytes <= kSpanLdsBytes;
  a.xt = P->xt; a.yt = P->yt; a.x_lo = P->x_lo; a.x_hi = P->x_hi; a.y_lo = P->y_lo; a.y_hi = P->y_hi;
  a.sx_lo = P->sx_lo; a.sx_hi = P->sx_hi;
  a.sy_lo = P->sy_lo; a.sy_hi = P->sy_hi;
  a.inv_cl = 1.0 / P->grid.cellLength;
  a.cand_off = P->cand_off; a.cand_list = P->cand_list;
  a.approx = P->approx; a.metric = P->metric; a.r = P->r; a.s_r = s_prefilter(P->r, 0);
  a.thr = P->metric == 0 ? a.s_r : a.r;
  a.qx0 = P->qx0; a.qy0 = P->qy0;
  a.qx = P->qx; a.qy = P->qy;
  a.npoly = P->npoly; a.ring_off = P->ring_off; a.vert_off = P->vert_off; a.vx = P->vx; a.vy = P->vy;
  a.bbox = P->bbox; a.ring_env = P->ring_env; a.rect = P->rect;
  a.brect = P->brect; a.g_layers = P->g_layers; a.c_layers = P->c_layers;
  return a;
}

// the deferred-test queue: one segment per scan block, each large enough for every point the
// block visits (a scan block visits at most 2 points per thread per grid sweep)
int ensure_queue(gf_range_plan* P, RangeArgs& a, int blocks, bool with_counts) {
  gf_ctx* ctx = P->ctx;
  const int64_t tstride = (int64_t)blocks * kBlock * 2;
  a.seg_cap = 2 * kBlock * ((a.n + tstride - 1) / tstride);
  a.drain_lanes = P->drain_lanes;
  const int64_t need = a.seg_cap * blocks;
  if (P->queue_cap < need || (with_counts && !P->jecnt)) {
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    void* old[] = {P->queue, P->queue_xy, P->jecnt, P->jecand};
    for (void* b : old)
      if (b) GF_HIP_CHECK(ctx, hipFree(b));
    P->queue = nullptr;
    P->queue_xy = nullptr;
    P->jecnt = nullptr;
    P->jecand = nullptr;
    P->queue_cap = 0;
    const int64_t cap = need;
    GF_HIP_CHECK(ctx, hipMalloc(&P->queue, sizeof(uint32_t) * (size_t)cap));
    GF_HIP_CHECK(ctx, hipMalloc(&P->queue_xy, 2 * sizeof(double) * (size_t)cap));
    if (with_counts) {
      GF_HIP_CHECK(ctx, hipMalloc(&P->jecnt, sizeof(uint32_t) * (size_t)cap));
      GF_HIP_CHECK(ctx, hipMalloc(&P->jecand, 4 * sizeof(uint32_t) * (size_t)cap));  // kJoinKeep
    }
    P->queue_cap = cap;
  }
  a.queue = P->queue;
  a.queue_xy = P->queue_xy;
  a.queue_count = P->queue_count;
  return GF_OK;
}

int scan_blocks_range(const gf_range_plan* P, int64_t n, bool span = false) {
  // every wave should run >= 2 pipeline stages of kRangeU tiles (range_kernel); at most 4
  // blocks per CU (the sweep in tools/bench_workloads.py: 1024 blocks best at 10M points), 2
  // for the span prefilter (C3, three windows in flight: 48.9 us per window at 512 blocks,
  // 51.5 at 1024; tools/gpu_r03_c3blocks.sh)
  int blocks = (int)std::min<int64_t>(std::max<int64_t>(n / (4 * 128 * 2 * 2), 1),
                                      (int64_t)P->ctx->num_cus * (span ? 2 : 4));
  if (P->scan_blocks > 0) blocks = P->scan_blocks;
  return std::min(blocks, 2048);  // queue segments / partial slots per window
}
}  // namespace

extern "C" int gf_range_run(gf_range_plan* P, const gf_points* pts, uint64_t* bitmap, uint64_t* multi,
                            int64_t* counts) {
  if (!P || !bitmap) return GF_ERR_ARG;
  if (P->join) return set_err(P->ctx, GF_ERR_ARG, "gf_range_run: a join plan (use gf_join_ppoly_run)");
  gf_ctx* ctx = P->ctx;
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, pts))) return st;
  if (pts->n == 0) {
    if (counts) GF_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), ctx->stream));
    return GF_OK;
  }
  RangeArgs a = range_args(P, pts, bitmap, multi);
  // Deferred tests pay a second launch; inline tests stall the waves holding candidate lanes.
  // Auto: defer while candidate cells are more than 5% of the non-none cells.
  const int64_t live = P->cls_cells[1] + P->cls_cells[2] + P->cls_cells[3];
  const bool can_defer = P->table_mode && (P->poly || !P->approx);
  const bool defer = can_defer && (P->defer_mode >= 2 || (P->defer_mode == 0 && P->cls_cells[1] * 20 > live));
  // span prefilter when the class spans cover at most a quarter of the grid (defer_mode 3
  // forces it): the stream skips the table, the block's queued points are classified after it
  // (the span prefilter's classification rounds read the span table from LDS only: it must fit)
  const bool span = defer && P->xt && P->span_bytes <= kSpanLdsBytes &&
                    (P->defer_mode == 3 || (P->defer_mode != 2 && P->span_frac <= 0.25));
  const int blocks = scan_blocks_range(P, pts->n, span);
  if (defer) {
    if ((st = ensure_queue(P, a, blocks, false))) return st;
    a.span_mode = span;
  }
  // the counts are summed by the last block of the window's last kernel (no finalize launch)
  a.counts = counts;
  GF_HIP_CHECK(ctx, launch_range(ctx, a, P->table_mode, P->poly, blocks));
  return GF_OK;
}

extern "C" int gf_range_run_batch(gf_range_plan* P, int32_t nwin, const gf_points* pts, uint64_t* const* bitmaps,
                                  int64_t* const* counts, uint32_t* const* idx, const int64_t* idx_cap,
                                  int64_t* const* idx_count) {
  if (!P || nwin < 1 || nwin > kRangeBatchMax || !pts || !bitmaps || !counts)
    return set_err(P ? P->ctx : nullptr, GF_ERR_ARG, "gf_range_run_batch: 1 <= nwin <= 16, pts / bitmaps / counts");
  if (P->join) return set_err(P->ctx, GF_ERR_ARG, "gf_range_run_batch: a join plan");
  gf_ctx* ctx = P->ctx;
  int st = bind(ctx);
  if (st) return st;
  int64_t nmax = 0;
  for (int32_t w = 0; w < nwin; ++w) {
    if ((st = check_points(ctx, &pts[w]))) return st;
    if (!bitmaps[w] || !counts[w]) return set_err(ctx, GF_ERR_ARG, "gf_range_run_batch: null bitmap / counts");
    if (idx && (pts[w].n > (int64_t)UINT32_MAX || !idx_cap || !idx_count || !idx_count[w] || idx_cap[w] < 0 ||
                (idx_cap[w] > 0 && !idx[w])))
      return set_err(ctx, GF_ERR_ARG, "gf_range_run_batch: index lists need idx, idx_cap, idx_count per window");
    nmax = std::max(nmax, pts[w].n);
  }
  if (!P->batch_partials) {  // tickets start at 0 and every finalising block resets its own
    GF_HIP_CHECK(ctx, hipMalloc(&P->batch_partials, sizeof(uint64_t) * (size_t)kRangeBatchMax * (kRangeTicketSlot + 1)));
    GF_HIP_CHECK(ctx, hipMemsetAsync(P->batch_partials, 0,
                                     sizeof(uint64_t) * (size_t)kRangeBatchMax * (kRangeTicketSlot + 1), ctx->stream));
  }
  RangeArgs a = range_args(P, &pts[0], bitmaps[0], nullptr);
  RangeBatch b{};
  for (int32_t w = 0; w < nwin; ++w)
    b.w[w] = RangeWin{pts[w].x, pts[w].y, pts[w].n, bitmaps[w], nullptr,
                      P->batch_partials + (size_t)w * (kRangeTicketSlot + 1), counts[w]};
  // blocks per window from the largest window (an empty window's blocks exit after the partials),
  // the whole launch held to ~4 blocks per CU as for one large window (r05 sweep, 16 windows of
  // 1M points: 488 blocks per window 3.7 us per window, 256: 3.4, 128: 3.3, 64: 3.25)
  int blocks = scan_blocks_range(P, nmax);
  if (P->scan_blocks == 0) blocks = std::max(1, std::min(blocks, (ctx->num_cus * 4 + nwin - 1) / nwin));
  GF_HIP_CHECK(ctx, launch_range_batch(ctx, a, b, nwin, P->table_mode, P->poly, blocks));
  if (!idx) return GF_OK;
  ExpandBatch e{};
  e.nwin = nwin;
  int64_t tiles = 0;
  for (int32_t w = 0; w < nwin; ++w) {
    e.bm[w] = bitmaps[w];
    e.n[w] = pts[w].n;
    e.idx[w] = idx[w];
    e.cap[w] = idx_cap[w];
    e.count[w] = idx_count[w];
    e.tile0[w] = (int32_t)tiles;
    tiles += std::max<int64_t>(expand_blocks((pts[w].n + 63) / 64), 1);  // >= 1: its block writes the count
  }
  e.tile0[nwin] = (int32_t)tiles;
  ExpandState es;
  if ((st = lookback_state(ctx, tiles, &es))) return st;
  GF_HIP_CHECK(ctx, launch_expand_batch(ctx->stream, e, es));
  ctx->expand_base += (unsigned long long)tiles;
  return GF_OK;
}

extern "C" int gf_join_ppoly_run(gf_range_plan* P, const gf_grid* ugrid, const gf_points* pts, uint32_t* pairs,
                                 int64_t cap, int64_t* npairs) {
  if (!P || !npairs || cap < 0 || !grid_ok(ugrid)) return GF_ERR_ARG;
  gf_ctx* ctx = P->ctx;
  if (!P->join) return set_err(ctx, GF_ERR_ARG, "gf_join_ppoly_run: not a join plan (gf_join_ppoly_plan_create)");
  const gf_grid& q = P->grid;
  if (ugrid->n != q.n || ugrid->minX != q.minX || ugrid->maxX != q.maxX || ugrid->minY != q.minY ||
      ugrid->maxY != q.maxY || ugrid->cellLength != q.cellLength)
    return set_err(ctx, GF_ERR_ARG, "gf_join_ppoly_run: the point grid must equal the polygon grid");
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, pts))) return st;
  *npairs = 0;
  if (pts->n == 0 || P->npoly == 0) return GF_OK;
  if (pts->n > (int64_t)UINT32_MAX) return set_err(ctx, GF_ERR_ARG, "gf_join_ppoly_run: window too large");
  RangeArgs a = range_args(P, pts, nullptr, nullptr);
  const int blocks = scan_blocks_range(P, pts->n);
  if ((st = ensure_queue(P, a, blocks, true))) return st;
  const int jblocks = blocks;  // one count/write block per scan block (its queue segment)
  GF_HIP_CHECK(ctx, launch_join_ppoly(ctx, a, blocks, jblocks, P->jecnt, P->jecand, P->jbtot, P->jtotal, pairs,
                                      pairs ? cap : 0, pairs && ((uintptr_t)pairs % 8 == 0)));
  unsigned long long total = 0;
  if ((st = read_scalar_sync(ctx, P->jtotal, &total))) return st;
  *npairs = (int64_t)total;
  if ((int64_t)total > cap || (total > 0 && !pairs)) return GF_ERR_CAPACITY;
  return GF_OK;
}

extern "C" int gf_join_ppoly(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* pts,
                             const gf_polygons* polys, double r, int approximate, int metric, uint32_t* pairs,
                             int64_t cap, int64_t* npairs) {
  gf_range_plan* P = nullptr;
  int st = gf_join_ppoly_plan_create(ctx, qgrid, polys, r, approximate, metric, &P);
  if (st) return st;
  st = gf_join_ppoly_run(P, ugrid, pts, pairs, cap, npairs);
  gf_range_plan_destroy(P);
  return st;
}

extern "C" int gf_range_plan_stats(const gf_range_plan* P, int64_t* none_cells, int64_t* candidate_cells,
                                   int64_t* guaranteed_cells, int64_t* inside_cells) {
  if (!P) return GF_ERR_ARG;
  if (none_cells) *none_cells = P->cls_cells[0];
  if (candidate_cells) *candidate_cells = P->cls_cells[1];
  if (guaranteed_cells) *guaranteed_cells = P->cls_cells[2];
  if (inside_cells) *inside_cells = P->cls_cells[3];
  return GF_OK;
}

extern "C" int gf_range_plan_set_tuning(gf_range_plan* P, int32_t scan_blocks, int32_t defer_mode) {
  if (!P || scan_blocks < 0 || scan_blocks > P->ctx->num_cus * 8 || defer_mode < 0 || defer_mode > 3)
    return GF_ERR_ARG;
  P->scan_blocks = scan_blocks;
  P->defer_mode = defer_mode;
  return GF_OK;
}

extern "C" int gf_range_plan_set_drain_lanes(gf_range_plan* P, int32_t lanes) {
  if (!P || lanes < 0 || lanes > 64) return GF_ERR_ARG;
  P->drain_lanes = lanes;
  return GF_OK;
}

extern "C" int gf_bitmap_to_indices(gf_ctx* ctx, const uint64_t* bitmap, int64_t n, uint32_t* idx, int64_t cap,
                                    int64_t* count) {
  if (!ctx || !bitmap || n < 0 || !count) return set_err(ctx, GF_ERR_ARG, "gf_bitmap_to_indices: bad argument");
  int st = bind(ctx);
  if (st) return st;
  const int64_t words = (n + 63) / 64;
  Arena ar;
  size_t o_pc = ar.take<uint32_t>(words + 1);
  size_t o_off = ar.take<uint32_t>(words + 1);
  size_t o_tmp = ar.take<uint32_t>(scan_tmp_elems(words));
  char* base = (char*)ctx_scratch(ctx, ar.off, &st);
  if (st) return st;
  uint32_t* pc = (uint32_t*)(base + o_pc);
  uint32_t* off = (uint32_t*)(base + o_off);
  uint32_t* tmp = (uint32_t*)(base + o_tmp);
  GF_HIP_CHECK(ctx, launch_word_popcounts(ctx->stream, bitmap, words, pc));
  GF_HIP_CHECK(ctx, launch_exclusive_scan(ctx->stream, pc, words, off, tmp));
  uint32_t total = 0;
  if (int e = read_scalar_sync(ctx, off + words, &total)) return e;
  *count = total;
  if ((int64_t)total > cap) return GF_ERR_CAPACITY;
  if (total) {
    if (!idx) return GF_ERR_ARG;
    GF_HIP_CHECK(ctx, launch_expand_bitmap(ctx->stream, bitmap, words, n, off, idx, cap));
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GF_OK;
}

// Ticket + epoch-tagged status words of the decoupled look-back kernels (expand_async, scan1)
// for a launch of `blocks` blocks; the caller adds `blocks` to ctx->expand_base after launching.
int gf::lookback_state(gf_ctx* ctx, int64_t blocks, gf::ExpandState* es) {
  if (!ctx->expand_ticket) {
    GF_HIP_CHECK(ctx, hipMalloc(&ctx->expand_ticket, sizeof(unsigned long long)));
    GF_HIP_CHECK(ctx, hipMemset(ctx->expand_ticket, 0, sizeof(unsigned long long)));
  }
  if (ctx->expand_status_cap < blocks) {  // epoch 0 is never used, so zeroed words read "not ready"
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->expand_status) GF_HIP_CHECK(ctx, hipFree(ctx->expand_status));
    ctx->expand_status = nullptr;
    const int64_t cap_b = std::max<int64_t>(blocks, 1024);
    GF_HIP_CHECK(ctx, hipMalloc(&ctx->expand_status, sizeof(unsigned long long) * (size_t)cap_b));
    GF_HIP_CHECK(ctx, hipMemset(ctx->expand_status, 0, sizeof(unsigned long long) * (size_t)cap_b));
    ctx->expand_status_cap = cap_b;
  }
  *es = gf::ExpandState{ctx->expand_ticket, ctx->expand_base, ctx->expand_status, 0};
  ctx->expand_epoch = (ctx->expand_epoch + 1) & 0x3FFFFFFu;
  if (ctx->expand_epoch == 0) ctx->expand_epoch = 1;
  es->epoch = ctx->expand_epoch;
  return GF_OK;
}

extern "C" int gf_bitmap_to_indices_async(gf_ctx* ctx, const uint64_t* bitmap, int64_t n, uint32_t* idx, int64_t cap,
                                          int64_t* count) {
  if (!ctx || !bitmap || n < 0 || n > (int64_t)UINT32_MAX || !count || cap < 0 || (cap > 0 && !idx))
    return set_err(ctx, GF_ERR_ARG, "gf_bitmap_to_indices_async: bad argument");
  int st = bind(ctx);
  if (st) return st;
  const int64_t words = (n + 63) / 64, blocks = expand_blocks(words);
  ExpandState es;
  if ((st = lookback_state(ctx, blocks, &es))) return st;
  GF_HIP_CHECK(ctx, launch_expand_bitmap_async(ctx->stream, bitmap, words, n, idx, cap, count, es));
  ctx->expand_base += (unsigned long long)(words > 0 ? blocks : 0);
  return GF_OK;
}

// ---------------------------------------------------------------------------------------
// kNN
// ---------------------------------------------------------------------------------------
extern "C" size_t gf_knn_result_bytes(int32_t k) {
  return sizeof(gf_knn_header) + (size_t)(k > 0 ? k : 0) * (sizeof(double) + 2 * sizeof(int64_t));
}

extern "C" void gf_knn_plan_destroy(gf_knn_plan* P) {
  if (!P) return;
  hipSetDevice(P->ctx->device);
  hipStreamSynchronize(P->ctx->stream);
  for (auto& L : P->lane) {
    if (L.st) hipFree(L.st);
    if (L.cand_d) hipFree(L.cand_d);
    if (L.cand_i) hipFree(L.cand_i);
    if (L.cand_o) hipFree(L.cand_o);
  }
  if (P->tmp_result) hipFree(P->tmp_result);
  if (P->host_result) hipHostFree(P->host_result);
  for (void* q : {(void*)P->ring_off, (void*)P->vert_off, (void*)P->vx, (void*)P->vy, (void*)P->ring_env})
    if (q) hipFree(q);
  for (uint32_t* m : P->maybe_i)  // one survivor buffer per stream (depth 4: three)
    if (m) hipFree(m);
  delete P;
}

static int knn_alloc_lane(gf_knn_plan* P, int j, int64_t cap) {
  gf_ctx* ctx = P->ctx;
  gf_knn_plan::Lane& L = P->lane[j];
  if (!L.st) {
    GF_HIP_CHECK(ctx, hipMalloc(&L.st, sizeof(KnnState)));
    GF_HIP_CHECK(ctx, hipMemset(L.st, 0, sizeof(KnnState)));
  }
  if (L.cand_d) hipFree(L.cand_d);
  if (L.cand_i) hipFree(L.cand_i);
  if (L.cand_o) hipFree(L.cand_o);
  L.cand_d = nullptr;
  L.cand_i = nullptr;
  L.cand_o = nullptr;
  GF_HIP_CHECK(ctx, hipMalloc(&L.cand_d, sizeof(double) * (size_t)cap));
  GF_HIP_CHECK(ctx, hipMalloc(&L.cand_i, sizeof(uint32_t) * (size_t)cap));
  GF_HIP_CHECK(ctx, hipMalloc(&L.cand_o, sizeof(int64_t) * (size_t)cap));
  return GF_OK;
}

static int knn_alloc_candidates(gf_knn_plan* P, int64_t cap) {
  int st;
  // queued windows may still read the old buffers (the k > kMaxK path queues without host reads)
  GF_HIP_CHECK(P->ctx, hipStreamSynchronize(P->ctx->stream));
  if (int e = sync_aux(P->ctx)) return e;
  for (int j = 0; j < (int)std::size(P->lane); ++j)  // lanes 1.. only once pipelining allocated them
    if ((j == 0 || P->lane[j].st) && (st = knn_alloc_lane(P, j, cap))) return st;
  P->cap = cap;
  return GF_OK;
}

extern "C" int gf_knn_pp_plan_create(gf_ctx* ctx, const gf_grid* g, double qx, double qy, double r, int32_t k,
                                     int metric, gf_knn_plan** out) {
  if (!ctx || !out || !grid_ok(g) || k < 1 || k > kMaxKLarge || (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, "gf_knn_pp_plan_create: bad argument (k must be in [1, 2^24])");
  *out = nullptr;
  int st = bind(ctx);
  if (st) return st;
  gf_knn_plan* P = new gf_knn_plan();
  P->ctx = ctx;
  P->grid = *g;
  P->qx = qx; P->qy = qy; P->r = r; P->k = k; P->metric = metric;
  const int32_t gl = guaranteed_layers(g->cellLength, r), cl = candidate_layers(g->cellLength, r);
  const int32_t qcx = cell_index(qx, g->minX, g->cellLength), qcy = cell_index(qy, g->minY, g->cellLength);
  P->qr = make_qrect(*g, qcx, qcy, gl, cl);  // PointPointKNNQuery.java:134-135
  auto fail = [&](int s) { gf_knn_plan_destroy(P); return s; };
  hipError_t e;
  if ((st = knn_alloc_candidates(P, (int64_t)1 << 20))) return fail(st);
  if ((e = hipMalloc(&P->tmp_result, gf_knn_result_bytes(k))) != hipSuccess) return fail(hip_err(ctx, e, "hipMalloc"));
  if ((e = hipHostMalloc(&P->host_result, gf_knn_result_bytes(k), hipHostMallocDefault)) != hipSuccess)
    return fail(hip_err(ctx, e, "hipHostMalloc"));
  P->scan_blocks = 0;
  P->large = k > kMaxK;
  *out = P;
  return GF_OK;
}

// PointPolygonKNNQuery.run(stream, queryPolygon, r, k) -- knn/PointPolygonKNNQuery.java:245-317:
// the C u G cells of the polygon's bbox cells (UniformGrid.java:193-206,399-411) as one rect
// pair (valid cells within c of the bbox rect; for g == 0 the bbox cells themselves, no
// validKey), the polygon on the device for the exact JTS distance.
extern "C" int gf_knn_ppoly_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_polygons* poly, double r,
                                        int32_t k, int approximate, int metric, gf_knn_plan** out) {
  if (!ctx || !out || !grid_ok(g) || !poly || poly->npoly != 1 || k < 1 || k > kMaxKLarge || (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, "gf_knn_ppoly_plan_create: bad argument (one polygon, 1 <= k <= 2^24)");
  *out = nullptr;
  const int32_t nrings = poly->ring_off[1] - poly->ring_off[0];
  if (poly->ring_off[0] != 0 || nrings < 1) return set_err(ctx, GF_ERR_ARG, "polygon without a shell");
  for (int32_t j = 0; j < nrings; ++j) {
    const int32_t v0 = poly->vert_off[j], v1 = poly->vert_off[j + 1];
    if (v1 - v0 < 4 || poly->vx[v0] != poly->vx[v1 - 1] || poly->vy[v0] != poly->vy[v1 - 1])
      return set_err(ctx, GF_ERR_ARG, "ring must be closed with >= 4 vertices");
  }
  int st = gf_knn_pp_plan_create(ctx, g, 0.0, 0.0, r, k, metric, out);
  if (st) return st;
  gf_knn_plan* P = *out;
  *out = nullptr;
  P->poly = 1;
  P->approx = approximate != 0;
  std::vector<double> renv(4 * (size_t)nrings);
  for (int32_t j = 0; j < nrings; ++j) {
    const int32_t v0 = poly->vert_off[j], v1 = poly->vert_off[j + 1];
    double mnx = poly->vx[v0], mxx = mnx, mny = poly->vy[v0], mxy = mny;
    for (int32_t v = v0 + 1; v < v1; ++v) {
      mnx = std::min(mnx, poly->vx[v]); mxx = std::max(mxx, poly->vx[v]);
      mny = std::min(mny, poly->vy[v]); mxy = std::max(mxy, poly->vy[v]);
    }
    renv[4 * j] = mnx; renv[4 * j + 1] = mxx; renv[4 * j + 2] = mny; renv[4 * j + 3] = mxy;
  }
  P->bbox[0] = renv[0]; P->bbox[1] = renv[2]; P->bbox[2] = renv[1]; P->bbox[3] = renv[3];  // shell envelope
  const int32_t gl = guaranteed_layers(g->cellLength, r), cl = candidate_layers(g->cellLength, r);
  const int64_t bx0 = cell_index(P->bbox[0], g->minX, g->cellLength), bx1 = cell_index(P->bbox[2], g->minX, g->cellLength);
  const int64_t by0 = cell_index(P->bbox[1], g->minY, g->cellLength), by1 = cell_index(P->bbox[3], g->minY, g->cellLength);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const int64_t n1 = g->n - 1;
  QueryRect q;
  q.minX = g->minX;
  q.minY = g->minY;
  if (cl > 0) {
    q.cgx = axis_iv(std::max<int64_t>(bx0 - cl, 0), std::min<int64_t>(bx1 + cl, n1), g->minX, g->cellLength);
    q.cgy = axis_iv(std::max<int64_t>(by0 - cl, 0), std::min<int64_t>(by1 + cl, n1), g->minY, g->cellLength);
  } else {
    q.cgx = q.cgy = {nan, nan};
  }
  if (gl > 0) {
    q.gx = axis_iv(std::max<int64_t>(bx0 - gl, 0), std::min<int64_t>(bx1 + gl, n1), g->minX, g->cellLength);
    q.gy = axis_iv(std::max<int64_t>(by0 - gl, 0), std::min<int64_t>(by1 + gl, n1), g->minY, g->cellLength);
  } else if (gl == 0) {  // the bbox cells themselves, without validKey
    q.gx = axis_iv(bx0, bx1, g->minX, g->cellLength);
    q.gy = axis_iv(by0, by1, g->minY, g->cellLength);
  } else {
    q.gx = q.gy = {nan, nan};
  }
  q.g_any = (gl >= 0) && !std::isnan(q.gx.lo) && !std::isnan(q.gy.lo);
  P->qr = q;
  const int32_t nverts = poly->vert_off[nrings];
  std::vector<int32_t> ro = {0, nrings}, vo(poly->vert_off, poly->vert_off + nrings + 1);
  std::vector<double> vx(poly->vx, poly->vx + nverts), vy(poly->vy, poly->vy + nverts);
  if ((st = upload(ctx, &P->ring_off, ro)) || (st = upload(ctx, &P->vert_off, vo)) || (st = upload(ctx, &P->vx, vx)) ||
      (st = upload(ctx, &P->vy, vy)) || (st = upload(ctx, &P->ring_env, renv))) {
    gf_knn_plan_destroy(P);
    return st;
  }
  *out = P;
  return GF_OK;
}

extern "C" int gf_knn_plan_set_capacity(gf_knn_plan* P, int64_t cap) {
  if (!P || cap < 2 || cap > (int64_t)1 << 31) return GF_ERR_ARG;
  int st = bind(P->ctx);
  if (st) return st;
  int fs = gf_knn_plan_flush(P);
  if (fs) return fs;
  hipStreamSynchronize(P->ctx->stream);
  return knn_alloc_candidates(P, cap & ~(int64_t)1);
}

extern "C" int gf_knn_plan_set_tuning(gf_knn_plan* P, int32_t scan_blocks, int32_t unroll, int32_t nontemporal) {
  if (!P || scan_blocks < 0 || unroll < 1 || unroll > 8) return GF_ERR_ARG;
  P->scan_blocks = scan_blocks;
  P->scan_unroll = unroll;
  P->scan_nt = nontemporal != 0;
  return GF_OK;
}

extern "C" int gf_knn_plan_set_index_base(gf_knn_plan* P, int64_t base) {
  if (!P || base < 0) return GF_ERR_ARG;
  P->idx_base = base;
  return GF_OK;
}

static int scan_blocks_for(gf_knn_plan* P, int64_t n) {
  int blocks = P->scan_blocks;
  if (blocks <= 0) {  // 4 blocks per CU measured best for the 1-pair nontemporal loop
    blocks = stream_blocks(P->ctx, (n + 1) / 2);
    blocks = std::min(blocks, P->ctx->num_cus * 4);
  }
  return blocks;
}

static KnnScanArgs scan_args(gf_knn_plan* P, int j, const gf_points* pts, int64_t begin, int64_t end, int use_state) {
  const gf_knn_plan::Lane& L = P->lane[j];
  KnnScanArgs s{};
  s.x = pts->x; s.y = pts->y; s.objID = pts->objID; s.begin = begin; s.end = end;
  s.qx = P->qx; s.qy = P->qy; s.qr = P->qr;
  s.T = P->r; s.s_pre = s_prefilter(P->r, P->metric);
  s.use_state = use_state; s.metric = P->metric; s.st = L.st;
  s.cand_d = L.cand_d; s.cand_i = L.cand_i; s.cand_o = L.cand_o; s.cap = (unsigned long long)P->cap;
  return s;
}

static KnnSelectArgs select_args(gf_knn_plan* P, int j, int use_state, int write_hint, void* result,
                                 int64_t idx_base) {
  const gf_knn_plan::Lane& L = P->lane[j];
  KnnSelectArgs q{};
  q.st = L.st; q.cand_d = L.cand_d; q.cand_i = L.cand_i; q.cand_o = L.cand_o;
  q.cap = (unsigned long long)P->cap;
  q.use_state = use_state; q.T = P->r; q.r = P->r; q.k = P->k; q.result = result;
  q.write_hint = write_hint; q.idx_base = idx_base;
  return q;
}

static KnnPolyArgs poly_args(gf_knn_plan* P, int j, const gf_points* pts, int64_t begin, int64_t end, int use_state,
                             int use_hint) {
  const gf_knn_plan::Lane& L = P->lane[j];
  KnnPolyArgs a{};
  a.x = pts->x; a.y = pts->y; a.objID = pts->objID; a.begin = begin; a.end = end;
  a.qr = P->qr;
  a.poly = PolyView{P->ring_off, P->vert_off, P->vx, P->vy, P->ring_env, P->metric};
  for (int i = 0; i < 4; ++i) a.bbox[i] = P->bbox[i];
  a.approx = P->approx; a.r = P->r; a.k = P->k; a.use_state = use_state; a.use_hint = use_hint;
  a.st = L.st; a.cand_d = L.cand_d; a.cand_i = L.cand_i; a.cand_o = L.cand_o; a.cap = (unsigned long long)P->cap;
  // one survivor buffer per stream (depth d >= 3: lane j runs on stream j % (d - 1); depth 2: lane j)
  a.maybe_i = P->maybe_i[P->pipeline >= 3 ? j % (P->pipeline - 1) : j];
  return a;
}

// the polygon scan's prefilter-survivor buffers (cap entries per lane)
static int poly_buffers(gf_knn_plan* P) {
  if (P->maybe_cap >= P->cap) return GF_OK;
  GF_HIP_CHECK(P->ctx, hipStreamSynchronize(P->ctx->stream));
  if (int e = sync_aux(P->ctx)) return e;
  for (auto& m : P->maybe_i) {
    if (m) hipFree(m);
    m = nullptr;
    GF_HIP_CHECK(P->ctx, hipMalloc(&m, sizeof(uint32_t) * (size_t)P->cap));
  }
  P->maybe_cap = P->cap;
  return GF_OK;
}

// scan + select of points [begin, end) on lane j, stream-ordered
static int knn_scan_select(gf_knn_plan* P, int j, const gf_points* pts, int64_t begin, int64_t end, int use_state,
                           int write_hint, void* result) {
  gf_ctx* ctx = P->ctx;
  if (P->poly) {
    int st = poly_buffers(P);
    if (st) return st;
    const KnnPolyArgs a = poly_args(P, j, pts, begin, end, use_state, 0);
    GF_HIP_CHECK(ctx, launch_knn_poly_scan(ctx, a, scan_blocks_for(P, (end - begin + 1) / 2)));
    GF_HIP_CHECK(ctx, launch_knn_select(ctx, select_args(P, j, use_state, write_hint, result, P->idx_base)));
    return GF_OK;
  }
  const KnnScanArgs s = scan_args(P, j, pts, begin, end, use_state);
  GF_HIP_CHECK(ctx, launch_knn_scan(ctx, s, scan_blocks_for(P, end - begin), P->scan_unroll, P->scan_nt));
  GF_HIP_CHECK(ctx, launch_knn_select(ctx, select_args(P, j, use_state, write_hint, result, P->idx_base)));
  return GF_OK;
}

// k > kMaxK (KNNQuery.java:216 takes any k): every candidate within r (T = r; lane 0's buffers
// hold the whole window, so nothing overflows), then two stable LSD radix sorts of the candidate
// permutation over 32-bit key fields (the K2 bucketing passes): (objID, d, idx) -> the first
// entry of each objID -> those by (d, objID, idx) -> the first k.  Grids and scratch are sized
// by the window (an upper bound of the candidate count) and every kernel reads the counts on
// the device: no host read, so windows queue back to back like the pipelined paths'.
static int knn_large(gf_knn_plan* P, const gf_points* pts, void* result) {
  gf_ctx* ctx = P->ctx;
  int st;
  const int64_t n = pts->n;
  if (P->cap < n && (st = knn_alloc_candidates(P, n))) return st;
  if (P->poly) {  // JTS point-polygon distances (prefilter + refine), T = r
    if ((st = poly_buffers(P))) return st;
    GF_HIP_CHECK(ctx, launch_knn_poly_scan(ctx, poly_args(P, 0, pts, 0, n, 0, 0), scan_blocks_for(P, (n + 1) / 2)));
  } else {
    const KnnScanArgs s = scan_args(P, 0, pts, 0, n, 0);  // T = r
    GF_HIP_CHECK(ctx, launch_knn_scan(ctx, s, scan_blocks_for(P, n), P->scan_unroll, P->scan_nt));
  }
  const gf_knn_plan::Lane& L = P->lane[0];
  const int64_t mm = std::max<int64_t>(n, 1);
  const int nb = (int)std::min<int64_t>(std::max<int64_t>((mm + radix_tile() - 1) / radix_tile() / 4, 1),
                                        (int64_t)radix_max_blocks(ctx->num_cus));
  const int64_t mat = (int64_t)256 * nb;  // 8-bit digits
  Arena ar;
  size_t o_k[2] = {ar.take<uint32_t>(mm), ar.take<uint32_t>(mm)};
  size_t o_p[2] = {ar.take<uint32_t>(mm), ar.take<uint32_t>(mm)};
  size_t o_c = ar.take<uint32_t>(2), o_m = ar.take<uint32_t>(mat), o_ms = ar.take<uint32_t>(mat + 1);
  char* base = (char*)ctx_scratch(ctx, ar.off, &st);
  if (st) return st;
  auto U32 = [&](size_t o) { return (uint32_t*)(base + o); };
  KnnLargeArgs a{};
  a.cd = L.cand_d; a.co = L.cand_o; a.ci = L.cand_i; a.k = P->k; a.T = P->r; a.idx_base = P->idx_base;
  a.result = result; a.m = mm; a.cnt = U32(o_c);
  a.lane_count = &L.st->count; a.lane_maybe = &L.st->maybe;
  GF_HIP_CHECK(ctx, launch_knn_large(ctx, 5, a));                 // counts
  int cur = 0;  // the permutation lives in o_p[cur]
  // stable sort of the first cnt[pass] entries of the permutation by key fields (least
  // significant first)
  auto sort_by = [&](int pass, std::initializer_list<int> fields) -> int {
    for (int f : fields) {
      a.perm = U32(o_p[cur]); a.field = f; a.keys = U32(o_k[0]); a.pass = pass;
      GF_HIP_CHECK(ctx, launch_knn_large(ctx, 1, a));
      for (int p = 0; p < 4; ++p) {  // 32 bits = 4 passes of 8
        RadixArgs r{};
        r.tile = radix_tile();
        r.n = mm; r.n_dev = a.cnt + pass;
        r.kin = U32(o_k[p & 1]); r.vin = U32(o_p[cur]);
        r.kout = U32(o_k[(p + 1) & 1]); r.vout = U32(o_p[cur ^ 1]);
        r.shift = p * 8; r.bits = 8; r.nblk = nb; r.M = U32(o_m); r.Ms = U32(o_ms);
        GF_HIP_CHECK(ctx, launch_radix(ctx, 0, r, nb));
        ExpandState es;
        if (int e = lookback_state(ctx, scan1_blocks(mat), &es)) return e;
        GF_HIP_CHECK(ctx, launch_scan1(ctx->stream, U32(o_m), mat, U32(o_ms), nullptr, 0, 0, es));
        ctx->expand_base += (unsigned long long)scan1_blocks(mat);
        GF_HIP_CHECK(ctx, launch_radix(ctx, 1, r, nb));
        cur ^= 1;
      }
    }
    return GF_OK;
  };
  a.perm = U32(o_p[cur]);
  GF_HIP_CHECK(ctx, launch_knn_large(ctx, 0, a));                 // identity permutation
  if ((st = sort_by(0, {0, 1, 2, 3, 4}))) return st;               // (objID, d, idx)
  a.perm = U32(o_p[cur]); a.out = U32(o_p[cur ^ 1]);
  GF_HIP_CHECK(ctx, launch_knn_large(ctx, 2, a));                 // first of each objID -> cnt[1]
  cur ^= 1;
  if ((st = sort_by(1, {0, 3, 4, 1, 2}))) return st;               // (d, objID, idx)
  a.perm = U32(o_p[cur]);
  GF_HIP_CHECK(ctx, launch_knn_large(ctx, 4, a));
  return GF_OK;
}

// stream s of a pipelined plan's windows in flight: 0 = the context stream, then the extra ones
static hipStream_t knn_stream(gf_ctx* ctx, hipStream_t main, int s) {
  return s == 0 ? main : (s == 1 ? ctx->aux : ctx->aux2);
}

static int knn_launch_sample(gf_knn_plan* P, int j, const gf_points* pts, int use_hint) {
  if (P->poly) {
    GF_HIP_CHECK(P->ctx, launch_knn_poly_sample(P->ctx, poly_args(P, j, pts, 0, pts->n, 1, use_hint)));
    return GF_OK;
  }
  KnnSampleArgs s{};
  s.x = pts->x; s.y = pts->y; s.n = pts->n; s.qx = P->qx; s.qy = P->qy; s.qr = P->qr;
  s.r = P->r; s.s_r = s_prefilter(P->r, P->metric); s.k = P->k; s.metric = P->metric; s.st = P->lane[j].st;
  s.use_hint = use_hint;
  GF_HIP_CHECK(P->ctx, launch_knn_sample(P->ctx, s));
  return GF_OK;
}

extern "C" int gf_knn_enqueue(gf_knn_plan* P, const gf_points* pts, void* result) {
  int merged = 0;
  return gf::knn_enqueue_merge(P, pts, result, nullptr, &merged);
}

int gf::knn_enqueue_merge(gf_knn_plan* P, const gf_points* pts, void* result, const KnnMergeArgs* merge,
                          int* merged) {
  *merged = 0;
  if (!P || !result) return GF_ERR_ARG;
  gf_ctx* ctx = P->ctx;
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, pts))) return st;
  if (pts->n > 0 && !pts->objID) return set_err(ctx, GF_ERR_ARG, "kNN needs objID");
  // k > kMaxK: the sorted path queues without host reads at every depth (its record is complete
  // in stream order, earlier than a pipelined plan promises)
  if (P->large) return knn_large(P, pts, result);
  if (P->pipeline >= 2 && P->k > kFusedSelectMaxK) {
    // k in (256, 512]: the select needs the standalone kernel's sort area, so it is not fused;
    // each window runs [sample] + scan + select on its lane, complete in stream order (earlier
    // than the depth promises).  Depth d >= 3 spreads windows over d - 1 streams with one lane
    // each: a lane's hint chain stays on one stream and consecutive windows' kernels overlap.
    const uint64_t kseq = P->seq++;
    const int S = P->pipeline >= 3 ? P->pipeline - 1 : 1, j = (int)(kseq % (uint64_t)S);
    hipStream_t main = ctx->stream;
    ctx->stream = knn_stream(ctx, main, j);
    const bool staged = pts->n >= kSampleMinN;  // the sample kernel takes the lane's hint when it has one
    int rc = staged ? knn_launch_sample(P, j, pts, P->use_hint) : GF_OK;
    if (rc == GF_OK) rc = knn_scan_select(P, j, pts, 0, pts->n, staged ? 1 : 0, staged && P->use_hint, result);
    ctx->stream = main;
    return rc;
  }
  if (P->pipeline >= 3) {
    // depth d >= 3, S = d - 1 streams: window k launches on stream k % S, scans lane k % 2S and
    // selects window k - S -- the previous launch on the SAME stream -- in block 0.  Every
    // dependency (window k - S's candidates, lane k % 2S's last select in launch k - 2S, its hint)
    // stays stream-ordered; consecutive windows' launches overlap (one's ramp-up under the
    // other's tail), S of them in flight.  Polygon queries: the fused launch is the prefilter
    // scan, the window's refine follows on the same stream (PointPolygonKNNQuery.java:245-317 per
    // window).  Window buffers must be complete when enqueued (no cross-stream wait is inserted).
    if (P->poly && (st = poly_buffers(P))) return st;
    const uint64_t S = (uint64_t)(P->pipeline - 1), kseq = P->seq++;
    const int j = (int)(kseq % (2 * S));
    hipStream_t main = ctx->stream;
    ctx->stream = knn_stream(ctx, main, (int)(kseq % S));
    int rc = GF_OK;
    do {
      const bool sample = pts->n >= kSampleMinN && (!P->use_hint || !P->lane_warm[j]);
      if (sample && (rc = knn_launch_sample(P, j, pts, 0))) break;
      P->lane_warm[j] = 1;
      KnnSelectArgs q{};
      int has_prev = 0;
      if (P->npq > 0 && P->pq[0].seq + S == kseq) {
        const gf_knn_plan::Pend e = P->pq[0];
        q = select_args(P, e.lane, 1, P->use_hint, e.result, e.idx_base);
        has_prev = 1;
        for (int t = 1; t < P->npq; ++t) P->pq[t - 1] = P->pq[t];
        --P->npq;
      }
      hipError_t he;
      if (P->poly)
        he = launch_knn_poly_fused(ctx, poly_args(P, j, pts, 0, pts->n, sample ? 2 : 1, 0), q, has_prev,
                                   scan_blocks_for(P, (pts->n + 1) / 2), nullptr);
      else
        he = launch_knn_fused(ctx, scan_args(P, j, pts, 0, pts->n, sample ? 2 : 1), q, has_prev,
                              scan_blocks_for(P, pts->n), P->scan_nt, merge);
      if (he != hipSuccess) { rc = hip_err(ctx, he, "launch_knn_fused"); break; }
      P->pq[P->npq++] = gf_knn_plan::Pend{j, result, P->idx_base, kseq};
    } while (0);
    ctx->stream = main;
    return rc;
  }
  if (P->pipeline == 2 && P->poly) {
    // polygon query: the prefilter scan of this window on lane j with the previous window's
    // select (other lane) in block 0, then this window's refine; its select rides the next launch
    const int j = (int)(P->seq++ & 1);
    if ((st = poly_buffers(P))) return st;
    const bool sample = pts->n >= kSampleMinN && (!P->use_hint || !P->lane_warm[j]);
    if (sample && (st = knn_launch_sample(P, j, pts, 0))) return st;
    P->lane_warm[j] = 1;
    const KnnPolyArgs a = poly_args(P, j, pts, 0, pts->n, sample ? 2 : 1, 0);
    KnnSelectArgs q{};
    const int has_prev = P->pend_lane >= 0;
    if (has_prev) q = select_args(P, P->pend_lane, 1, P->use_hint, P->pend_result, P->pend_idx_base);
    const bool fold = merge && merge->nrec > 0 && has_prev && P->k <= kFusedMergeMaxK;
    GF_HIP_CHECK(ctx, launch_knn_poly_fused(ctx, a, q, has_prev, scan_blocks_for(P, (pts->n + 1) / 2),
                                           fold ? merge : nullptr));
    *merged = fold ? 1 : 0;
    P->pend_lane = j;
    P->pend_result = result;
    P->pend_idx_base = P->idx_base;
    return GF_OK;
  }
  if (P->pipeline == 2) {
    // one fused launch: scan this window on lane j (threshold = the lane's hint), select the
    // pending previous window on the other lane in block 0
    const int j = (int)(P->seq++ & 1);
    // a lane's first window (or hints off): sample the threshold instead of guessing r
    const bool sample = pts->n >= kSampleMinN && (!P->use_hint || !P->lane_warm[j]);
    if (sample && (st = knn_launch_sample(P, j, pts, 0))) return st;
    P->lane_warm[j] = 1;
    const KnnScanArgs s = scan_args(P, j, pts, 0, pts->n, sample ? 2 : 1);
    KnnSelectArgs q{};
    const int has_prev = P->pend_lane >= 0;
    if (has_prev) q = select_args(P, P->pend_lane, 1, P->use_hint, P->pend_result, P->pend_idx_base);
    const bool fold = merge && merge->nrec > 0 && has_prev && P->k <= kFusedMergeMaxK;
    GF_HIP_CHECK(ctx, launch_knn_fused(ctx, s, q, has_prev, scan_blocks_for(P, pts->n), P->scan_nt,
                                       fold ? merge : nullptr));
    *merged = fold ? 1 : 0;
    P->pend_lane = j;
    P->pend_result = result;
    P->pend_idx_base = P->idx_base;  // the index base in force when this window was enqueued
    return GF_OK;
  }
  // threshold: the previous window's hint (continuous query) or the sample; tiny windows
  // scan to r
  const bool staged = pts->n >= kSampleMinN;
  if (staged && (st = knn_launch_sample(P, 0, pts, P->use_hint))) return st;
  return knn_scan_select(P, 0, pts, 0, pts->n, staged ? 1 : 0, staged && P->use_hint, result);
}

extern "C" int gf_knn_plan_flush(gf_knn_plan* P) {
  if (!P) return GF_ERR_ARG;
  if (P->pipeline >= 3) {
    if (P->npq == 0) return P->k > kFusedSelectMaxK ? gf_ctx_join(P->ctx) : GF_OK;  // mid k: the other streams
    gf_ctx* ctx = P->ctx;
    int st = bind(ctx);
    if (st) return st;
    hipStream_t main = ctx->stream;
    for (int e = 0; e < P->npq; ++e) {
      const gf_knn_plan::Pend& w = P->pq[e];
      ctx->stream = knn_stream(ctx, main, (int)(w.seq % (uint64_t)(P->pipeline - 1)));
      hipError_t he = launch_knn_select(ctx, select_args(P, w.lane, 1, P->use_hint, w.result, w.idx_base));
      ctx->stream = main;
      if (he != hipSuccess) return hip_err(ctx, he, "launch_knn_select");
    }
    P->npq = 0;
    // every window of the plan is complete in the context stream's order from here on
    return gf_ctx_join(ctx);
  }
  if (P->pend_lane < 0) return GF_OK;
  gf_ctx* ctx = P->ctx;
  int st = bind(ctx);
  if (st) return st;
  GF_HIP_CHECK(ctx, launch_knn_select(ctx, select_args(P, P->pend_lane, 1, P->use_hint, P->pend_result,
                                                       P->pend_idx_base)));
  P->pend_lane = -1;
  P->pend_result = nullptr;
  return GF_OK;
}

extern "C" int gf_knn_plan_set_pipeline(gf_knn_plan* P, int depth) {
  if (!P || depth < 1 || depth > 4) return GF_ERR_ARG;
  gf_ctx* ctx = P->ctx;
  int st = bind(ctx);
  if (st || (st = gf_knn_plan_flush(P))) return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (int e = sync_aux(ctx)) return e;
  // k > 512 plans return through knn_large (lane 0, stream-ordered) before any pipelined path:
  // no extra lanes, no second stream
  const int lanes = depth >= 3 ? 2 * (depth - 1) : depth;
  for (int j = 1; !P->large && j < lanes; ++j)
    if (!P->lane[j].st && (st = knn_alloc_lane(P, j, P->cap))) return st;
  if (depth >= 3 && !P->large && !ctx->aux)
    GF_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
  if (depth >= 4 && !P->large && !ctx->aux2)
    GF_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->aux2, hipStreamNonBlocking));
  P->pipeline = depth;
  P->seq = 0;
  for (int& w : P->lane_warm) w = 0;
  P->npq = 0;
  return GF_OK;
}

extern "C" int gf_knn_plan_set_hint(gf_knn_plan* P, int enable) {
  if (!P) return GF_ERR_ARG;
  int st = bind(P->ctx);
  if (st) return st;
  P->use_hint = enable != 0;
  if ((st = gf_knn_plan_flush(P))) return st;
  GF_HIP_CHECK(P->ctx, hipStreamSynchronize(P->ctx->stream));
  for (auto& L : P->lane)
    if (L.st) GF_HIP_CHECK(P->ctx, hipMemset(&L.st->hint_T, 0, sizeof(double)));
  for (int& w : P->lane_warm) w = 0;
  return GF_OK;
}

namespace {
struct Ent { double d; int64_t o, i; };
void merge_lists(int32_t k, std::vector<Ent>& all, int64_t* oo, double* od, int64_t* oi, int32_t* n_out) {
  std::sort(all.begin(), all.end(), [](const Ent& a, const Ent& b) {
    if (a.d != b.d) return a.d < b.d;
    if (a.o != b.o) return a.o < b.o;
    return a.i < b.i;
  });
  std::unordered_set<int64_t> seen;
  int32_t n = 0;
  for (const Ent& e : all) {
    if (n >= k) break;
    if (!seen.insert(e.o).second) continue;
    if (oo) oo[n] = e.o;
    if (od) od[n] = e.d;
    if (oi) oi[n] = e.i;
    ++n;
  }
  *n_out = n;
}
}  // namespace

extern "C" int gf_knn_merge_host(int32_t k, int32_t nlists, const int32_t* counts, const int64_t* objID,
                                 const double* dist, const int64_t* idx, int64_t* oo, double* od, int64_t* oi,
                                 int32_t* n_out) {
  if (k < 1 || nlists < 0 || !n_out || (nlists > 0 && (!counts || !objID || !dist))) return GF_ERR_ARG;
  std::vector<Ent> all;
  int64_t off = 0;
  for (int32_t l = 0; l < nlists; ++l)
    for (int32_t j = 0; j < counts[l]; ++j, ++off) all.push_back({dist[off], objID[off], idx ? idx[off] : 0});
  merge_lists(k, all, oo, od, oi, n_out);
  return GF_OK;
}

// Re-evaluation of a flagged window: first the sample path with the hint ignored; if that is
// still inconclusive, the exact sorted path over every candidate within r (knn_large) -- on the
// device, like every other result.
static int knn_fallback(gf_knn_plan* P, const gf_points* pts, int64_t* oo, double* od, int64_t* oi, int32_t* n_out) {
  gf_ctx* ctx = P->ctx;
  const size_t rb = gf_knn_result_bytes(P->k);
  const gf_knn_header* h = (const gf_knn_header*)P->host_result;
  auto fetch = [&]() -> int {
    GF_HIP_CHECK(ctx, hipMemcpyAsync(P->host_result, P->tmp_result, rb, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return GF_OK;
  };
  int st = gf_knn_plan_flush(P);  // lane 0 is free afterwards
  if (st) return st;
  if (!P->poly && pts->n >= kSampleMinN) {
    if ((st = knn_launch_sample(P, 0, pts, 0)) ||
        (st = knn_scan_select(P, 0, pts, 0, pts->n, 1, P->use_hint, P->tmp_result)) || (st = fetch()))
      return st;
    if (h->status == 0) return gf_knn_decode(P, pts, P->host_result, oo, od, oi, n_out);
  }
  if ((st = knn_large(P, pts, P->tmp_result)) || (st = fetch())) return st;
  if (h->status != 0) return set_err(ctx, GF_ERR_HIP, "kNN exact path did not converge");
  return gf_knn_decode(P, pts, P->host_result, oo, od, oi, n_out);
}

extern "C" int gf_knn_decode(gf_knn_plan* P, const gf_points* pts, const void* result_host, int64_t* oo,
                             double* od, int64_t* oi, int32_t* n_out) {
  if (!P || !result_host || !n_out) return GF_ERR_ARG;
  const gf_knn_header* h = (const gf_knn_header*)result_host;
  if (h->status == 0) {
    const double* d = (const double*)(h + 1);
    const int64_t* o = (const int64_t*)(d + h->k);
    const int64_t* i = o + h->k;
    for (int32_t j = 0; j < h->n; ++j) {
      if (oo) oo[j] = o[j];
      if (od) od[j] = d[j];
      if (oi) oi[j] = i[j];
    }
    *n_out = h->n;
    return GF_OK;
  }
  int st = bind(P->ctx);
  if (st) return st;
  if ((st = check_points(P->ctx, pts))) return st;
  return knn_fallback(P, pts, oo, od, oi, n_out);
}

extern "C" int gf_knn_run(gf_knn_plan* P, const gf_points* pts, int64_t* oo, double* od, int64_t* oi,
                          int32_t* n_out) {
  if (!P || !n_out) return GF_ERR_ARG;
  gf_ctx* ctx = P->ctx;
  // the synchronous call may get a window the caller produced on the context stream just now:
  // order the second stream after it (nothing to overlap with in a synchronous call)
  int st = P->pipeline >= 3 ? gf_ctx_fork(ctx) : GF_OK;
  if (st) return st;
  st = gf_knn_enqueue(P, pts, P->tmp_result);
  if (st || (st = gf_knn_plan_flush(P))) return st;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(P->host_result, P->tmp_result, gf_knn_result_bytes(P->k), hipMemcpyDeviceToHost,
                                   ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return gf_knn_decode(P, pts, P->host_result, oo, od, oi, n_out);
}

// k > kMaxK merges rank entries in global scratch (the context's, stream-ordered)
static int merge_scratch(gf_ctx* ctx, int32_t k, int32_t nrec, int32_t nwin, void** out) {
  *out = nullptr;
  if (k <= kMaxK) return GF_OK;
  int st = GF_OK;
  *out = ctx_scratch(ctx, merge_any_bytes(nrec, k) * (size_t)nwin, &st);
  return st;
}

extern "C" int gf_knn_merge_dev(gf_ctx* ctx, int32_t k, const void* records, int32_t nrec, void* result) {
  if (!ctx || k < 1 || k > kMaxKLarge || nrec < 1 || nrec > 64 || !records || !result)
    return set_err(ctx, GF_ERR_ARG, "gf_knn_merge_dev: need 1 <= nrec <= 64 and 1 <= k <= 2^24");
  int st = bind(ctx);
  if (st) return st;
  const size_t rb = gf_knn_result_bytes(k);
  void* scratch;
  if ((st = merge_scratch(ctx, k, nrec, 1, &scratch))) return st;
  GF_HIP_CHECK(ctx, launch_knn_merge(ctx, k, records, nrec, rb, 1, 0, result, 0, 0, scratch));
  return GF_OK;
}

extern "C" int gf_knn_merge_dev_batch(gf_ctx* ctx, int32_t k, const void* records, int32_t nrec, int32_t nwin,
                                      int32_t layout, void* results) {
  const int foreign = (layout & GF_MERGE_FOREIGN_KEYS) != 0;
  layout &= ~GF_MERGE_FOREIGN_KEYS;
  if (!ctx || k < 1 || k > kMaxKLarge || nrec < 1 || nrec > 64 || nwin < 1 || nwin > 65535 || !records || !results ||
      (layout != GF_MERGE_SHARD_MAJOR && layout != GF_MERGE_WINDOW_MAJOR))
    return set_err(ctx, GF_ERR_ARG, "gf_knn_merge_dev_batch: bad argument");
  int st = bind(ctx);
  if (st) return st;
  const size_t rb = gf_knn_result_bytes(k);
  // shard-major = all_gather of each rank's [nwin] records: record (shard s, window w) at (s*nwin + w)*rb
  const size_t rec_stride = layout == GF_MERGE_SHARD_MAJOR ? (size_t)nwin * rb : rb;
  const size_t win_stride = layout == GF_MERGE_SHARD_MAJOR ? rb : (size_t)nrec * rb;
  void* scratch;
  if ((st = merge_scratch(ctx, k, nrec, nwin, &scratch))) return st;
  GF_HIP_CHECK(ctx, launch_knn_merge(ctx, k, records, nrec, rec_stride, nwin, win_stride, results, rb, foreign,
                                     scratch));
  return GF_OK;
}

// ---------------------------------------------------------------------------------------
// join
// ---------------------------------------------------------------------------------------
// total_out == nullptr: synchronous (*npairs from a pinned readback); else asynchronous (the
// packing kernel writes the count to total_out; *npairs untouched)
static int join_pp_impl(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* ord,
                        const gf_points* qry, double r, int approximate, int metric, uint32_t* pairs, int64_t cap,
                        int64_t* npairs, unsigned long long* total_out) {
  if (!ctx || !grid_ok(ugrid) || !grid_ok(qgrid) || !npairs || (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, "gf_join_pp: bad argument");
  ctx->join_async_done = 0;
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, ord)) || (st = check_points(ctx, qry))) return st;
  *npairs = 0;
  int64_t c;
  if (r == 0) {
    c = -1;  // getNeighboringCells: every grid cell (UniformGrid.java:264-266)
  } else {
    c = candidate_layers(qgrid->cellLength, r);
    if (c <= 0) return set_err(ctx, GF_ERR_LAYERS, "candidateNeighboringLayers cannot be 0 or less");
  }
  const int64_t no = ord->n, nq = qry->n;
  if (no == 0 || nq == 0) return GF_OK;
  const int64_t qn = qgrid->n, W = qn + 2, bins = W * W;
  if (bins >= (int64_t)INT32_MAX / 2) return set_err(ctx, GF_ERR_ARG, "query grid too large");
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>((no + kBlock - 1) / kBlock, 1), (int64_t)ctx->num_cus * 8);
  // row-bucketed path (k_join.hip): bucket the ordinary side by cell row, probe per task
  // (pairs carry u32 sorted slots or query indices with the top bit as a flag: nq < 2^31)
  const bool rowpath = c >= 0 && 2 * c + 1 <= kJoinMaxRows && qn + 8 <= 8192 && nq < ((int64_t)1 << 31) &&
                       !ctx->join_legacy;
  // fine path (k_join.hip): c == 1, exact distances, one grid for both sides
  int32_t f = 1;
  if (rowpath && c == 1 && !approximate && !ctx->join_coarse && ugrid->n == qgrid->n && ugrid->minX == qgrid->minX &&
      ugrid->minY == qgrid->minY && ugrid->cellLength == qgrid->cellLength) {
    const double ext = (double)qn * qgrid->cellLength;
    const double maxabs = std::max({std::fabs(qgrid->minX), std::fabs(qgrid->minY), std::fabs(qgrid->minX + ext),
                                    std::fabs(qgrid->minY + ext)});
    f = join_fine_factor(qgrid->cellLength, r, (int32_t)qn, maxabs);
  }
  const int64_t fbins = (int64_t)f * W * f * W;  // q_off entries (sub-cells on the fine path)
  Arena ar;
  size_t o_keys = ar.take<uint32_t>(nq), o_qcx = ar.take<int32_t>(nq), o_qcy = ar.take<int32_t>(nq);
  size_t o_hist = ar.take<uint32_t>(bins), o_off = ar.take<uint32_t>(std::max(bins, fbins) + 1), o_cur = ar.take<uint32_t>(std::max(bins, fbins));
  size_t o_tmp = ar.take<uint32_t>(std::max(scan_tmp_elems(bins), scan_tmp_elems(blocks)));
  size_t o_sqx = ar.take<double>(nq), o_sqy = ar.take<double>(nq);
  size_t o_sqcx = ar.take<int32_t>(nq), o_sqcy = ar.take<int32_t>(nq), o_sqi = ar.take<uint32_t>(nq);
  size_t o_cnt = ar.take<uint32_t>(blocks), o_boff = ar.take<uint32_t>(blocks + 1);
  // bucketing grids: one block per CU in the scatter (its tile buffers fill the LDS), split
  // between the sides by their point counts
  const int qblk = (int)std::max<int64_t>(1, std::min<int64_t>(nq / 8192 + 1, (int64_t)ctx->num_cus * nq / (no + nq)));
  const int sblocks = (int)std::max<int64_t>(1, std::min<int64_t>(no / 8192 + 1, (int64_t)ctx->num_cus - qblk));
  const int64_t nrows = qn;  // ordinary-side rows
  // experiment: only the query side bucketed, the ordinary points streamed (fine path)
  const bool stream = rowpath && f > 1 && ctx->join_stream;
  const int64_t qmat = rowpath ? W * 2 * qblk : 1, mat = rowpath && !stream ? nrows * 2 * sblocks : 1;  // kHistSplit = 2
  size_t o_cat = ar.take<uint32_t>(qmat + mat), o_cats = ar.take<uint32_t>(qmat + mat + 1);
  size_t o_txy = ar.take<double>(rowpath ? 2 * nq : 1), o_tidx = ar.take<uint32_t>(rowpath ? nq : 1);
  size_t o_roff = ar.take<uint32_t>(nrows + 1), o_toff = ar.take<uint32_t>(nrows + 1);
  size_t o_gcnt = ar.take<unsigned long long>(2);  // -, total
  // output (JoinOut): the persistent probe's waves, one chunk each at a time, sized from the last
  // join's pairs per point so that a window takes ~8 chunks per wave: few atomics, small holes
  // (GF_JOIN_BAND_PER_CU, A/B testing only: band probe blocks per CU -- the product's 160 KB
  // block fills a CU's LDS; an experiment build with an 80 KB block can hold two)
  const char* pcu = std::getenv("GF_JOIN_BAND_PER_CU");
  const int64_t per_cu = pcu && *pcu >= '1' && *pcu <= '4' ? *pcu - '0' : 1;
  const int64_t probe_blocks = std::max(8, ctx->num_cus / 8 * 8) * per_cu;
  const int64_t nwaves = probe_blocks * (kJoinThreads / 64);
  // pairs per point of the last join: its exact count (sync) or the fix-up's pinned copy (async)
  double ppp = ctx->join_ppp > 0 ? ctx->join_ppp : 1.0;
  if (ctx->join_hint && ctx->join_hint_no > 0) {
    const unsigned long long h = *(volatile unsigned long long*)ctx->join_hint;
    if (h > 0) ppp = (double)h / (double)ctx->join_hint_no;
  }
  // output: the band probe fills per-block regions (JoinOut.regions); the row probe and the
  // streaming experiment take per-wave chunks (one device atomic each, one hole per wave).
  // fine path: the band probe (k_join.hip) unless the row probe is asked for (A/B testing)
  const char* renv = std::getenv("GF_JOIN_ROWPROBE");
  const bool band = rowpath && f > 1 && !stream && !(renv && *renv == '1') && probe_blocks <= 1016;
  const int64_t ntails = nwaves;
  int64_t chunk = 256;
  while (chunk < 65536 && (double)chunk * ntails * 8 < ppp * (double)no)
    chunk <<= 1;
  if (const char* e = std::getenv("GF_JOIN_CHUNK")) {  // testing / tuning: a fixed chunk (power of 2)
    const int64_t v = std::atoll(e);
    if (v >= 64 && v <= 65536 && (v & (v - 1)) == 0) chunk = v;
  }
  // band probe regions: e_lim bounds the regions' total E (hint x 1.125 + 1024 per block; the
  // regions come from the last call's per-block pairs x 1.03 + 256, so they are scaled down only
  // when the history and the hint disagree).  Positions used = E + the overflow area, and the
  // overflow (pairs past their block's region) is at most the pair count T, so every position is
  // below E + T <= e_lim + cap whenever T <= cap: a spill of e_lim past cap backs them all, and a
  // window whose pairs fit is never answered GF_ERR_CAPACITY, whatever the regions' sizing
  // (VERDICT r04 item 6).  The spill is scratch written only by overflowing blocks (HBM capacity,
  // not traffic); r06: e_lim no longer takes max(cap, ...), which made every call reserve a
  // second cap-sized buffer.
  const double t_hint = ppp * (double)no;
  const uint64_t ucap = pairs ? (uint64_t)std::max<int64_t>(cap, 0) : 0;
  const uint64_t e_lim = (uint64_t)(1.125 * t_hint) + (uint64_t)probe_blocks * 1024;
  const uint64_t spill_cap = band ? (ucap == 0 ? 0 : e_lim + std::max<uint64_t>(65536, (uint64_t)(t_hint / 16)))
                                  : (uint64_t)(ntails * chunk);
  size_t o_spill = ar.take<uint64_t>(rowpath ? std::max<uint64_t>(spill_cap, 1) : 1);
  size_t o_bcnt = ar.take<uint64_t>(probe_blocks), o_bsl = ar.take<uint64_t>(probe_blocks);
  size_t o_tb = ar.take<uint64_t>(nwaves), o_tf = ar.take<uint32_t>(nwaves);
  size_t o_hs = ar.take<uint64_t>(nwaves + 1), o_hp = ar.take<uint64_t>(nwaves + 2);
  size_t o_ss = ar.take<uint64_t>(nwaves + 2), o_sp = ar.take<uint64_t>(nwaves + 3), o_fc = ar.take<uint32_t>(2);
  size_t o_soxy = ar.take<double>(rowpath ? 2 * no : 1), o_soidx = ar.take<uint32_t>(rowpath ? no : 1);
  char* base = (char*)ctx_scratch(ctx, ar.off, &st);
  if (st) return st;
  auto U32 = [&](size_t o) { return (uint32_t*)(base + o); };
  auto I32 = [&](size_t o) { return (int32_t*)(base + o); };
  auto F64 = [&](size_t o) { return (double*)(base + o); };
  hipStream_t s = ctx->stream;
  if (rowpath) {
    if (!ctx->join_gctr) {  // the output counter (the fix-up resets it) and the size hint
      GF_HIP_CHECK(ctx, hipMalloc(&ctx->join_gctr, sizeof(unsigned long long)));
      GF_HIP_CHECK(ctx, hipMemset(ctx->join_gctr, 0, sizeof(unsigned long long)));
      void* h = nullptr;
      if (gf_pinned_alloc(sizeof(unsigned long long), &h) == GF_OK) {
        ctx->join_hint = (unsigned long long*)h;
        *ctx->join_hint = 0ull;
      }
    }
    ctx->join_hint_no = no;
    JoinQueryArgs q{};
    q.qx = qry->x; q.qy = qry->y; q.nq = nq;
    q.minX = qgrid->minX; q.minY = qgrid->minY; q.cl = qgrid->cellLength; q.qn = (int32_t)qn;
    q.nblk = qblk; q.qmat = U32(o_cat); q.qmat_scan = U32(o_cats);
    q.txy = F64(o_txy); q.tidx = U32(o_tidx); q.q_off = U32(o_off);
    q.sqx = F64(o_sqx); q.sqy = F64(o_sqy); q.sqcx = I32(o_sqcx); q.sqcy = I32(o_sqcy); q.sqidx = U32(o_sqi);
    q.f = f; q.fs = (double)f / qgrid->cellLength;
    JoinRowArgs j{};
    j.ox = ord->x; j.oy = ord->y; j.no = no;
    j.u_minX = ugrid->minX; j.u_minY = ugrid->minY; j.u_cl = ugrid->cellLength;
    j.qn = (int32_t)qn; j.c = c; j.q_off = U32(o_off);
    j.sqx = F64(o_sqx); j.sqy = F64(o_sqy); j.sqcx = I32(o_sqcx); j.sqcy = I32(o_sqcy); j.sqidx = U32(o_sqi);
    j.approx = approximate != 0; j.metric = metric; j.r = r; j.s_r = s_prefilter(r, 0);
    j.nblk = stream ? 0 : sblocks; j.nrows = stream ? 0 : (int32_t)nrows;
    j.row_mat = U32(o_cat) + qmat; j.row_mat_scan = U32(o_cats) + qmat; j.mat_base = (uint32_t)nq;
    j.row_off_w = U32(o_roff); j.row_off = U32(o_roff); j.task_off_w = U32(o_toff); j.task_off = U32(o_toff);
    j.soxy = (double*)(base + o_soxy); j.soidx = U32(o_soidx);
    unsigned long long* cnt2 = (unsigned long long*)(base + o_gcnt);
    JoinOut& o = j.out;
    o.pairs = pairs;
    o.cap = pairs ? (uint64_t)std::max<int64_t>(cap, 0) : 0;
    o.aligned = ((uintptr_t)pairs & 7) == 0;
    o.chunk = (uint32_t)chunk;
    o.spill = (uint2*)(base + o_spill);
    o.spill_cap = spill_cap;
    if (band) {
      if (!ctx->join_hist) {  // zero: no history (the first call's regions come from ppp)
        GF_HIP_CHECK(ctx, hipMalloc(&ctx->join_hist, sizeof(uint64_t) * (3 * (size_t)probe_blocks + 1)));
        GF_HIP_CHECK(ctx, hipMemsetAsync(ctx->join_hist, 0, sizeof(uint64_t) * (3 * (size_t)probe_blocks + 1), s));
        GF_HIP_CHECK(ctx, hipMalloc(&ctx->join_ovf, 2 * sizeof(unsigned long long)));  // overflow, ticket
        GF_HIP_CHECK(ctx, hipMemsetAsync(ctx->join_ovf, 0, 2 * sizeof(unsigned long long), s));
      }
      o.regions = 1;
      o.bcount = (uint64_t*)(base + o_bcnt);
      o.bslice = (uint64_t*)(base + o_bsl);
      o.hist = ctx->join_hist;
      o.ovf = ctx->join_ovf;
      o.e_lim = e_lim;
      o.ppp = ppp;
    }
    o.gctr = ctx->join_gctr;
    o.tail_base = (uint64_t*)(base + o_tb);
    o.tail_fill = U32(o_tf);
    o.nwaves = (uint32_t)(band ? probe_blocks : ntails);  // tails: the probe's waves, or its blocks / regions
    j.f = f; j.fs = (double)f / ugrid->cellLength;
    j.lds_budget = join_probe_budget(nq, qn, c, f);
    // (1) row histograms of both sides, (2) one scan of both matrices, (3) write-combined row
    // scatter of both sides, (4) query rows sorted by (sub-)cell + ordinary row / task offsets,
    // (5) probe (its last block scans the task counts), (6) packing
    GF_HIP_CHECK(ctx, launch_join_rows(ctx, j, q, 0));
    ExpandState es;
    if ((st = lookback_state(ctx, scan1_blocks(qmat + mat), &es))) return st;
    GF_HIP_CHECK(ctx, launch_scan1(s, U32(o_cat), qmat + mat, U32(o_cats), nullptr, 0, 0, es));
    ctx->expand_base += (unsigned long long)scan1_blocks(qmat + mat);
    GF_HIP_CHECK(ctx, launch_join_rows(ctx, j, q, 1));
    GF_HIP_CHECK(ctx, launch_join_rows(ctx, j, q, 2));
    JoinFixup fx{};
    fx.o = j.out;
    fx.total = total_out ? total_out : cnt2 + 1;
    fx.hint = ctx->join_hint;
    fx.hole_start = (uint64_t*)(base + o_hs); fx.hole_pref = (uint64_t*)(base + o_hp);
    fx.seg_start = (uint64_t*)(base + o_ss); fx.seg_pref = (uint64_t*)(base + o_sp);
    fx.counts = U32(o_fc);
    if (band) {  // its last block prepares the fix-up (fx)
      j.fx = fx;
      j.ticket = ctx->join_ovf + 1;
      GF_HIP_CHECK(ctx, launch_join_band(ctx, j, (int)probe_blocks));
    } else if (stream) {
      j.out.nwaves = (uint32_t)nwaves;  // the stream grid: kBlock-thread blocks, same wave count
      GF_HIP_CHECK(ctx, launch_join_stream(ctx, j));
    } else {
      GF_HIP_CHECK(ctx, launch_join_rows(ctx, j, q, 3));
    }
    fx.o = j.out;  // (the streaming experiment changed its wave count)
    GF_HIP_CHECK(ctx, launch_join_fixup(ctx, fx));
    if (total_out) {  // the caller reads *total_out stream-ordered
      ctx->join_async_done = 1;
      return GF_OK;
    }
    unsigned long long total = 0;
    if (int e = read_scalar_sync(ctx, cnt2 + 1, &total)) return e;
    *npairs = (int64_t)total;
    ctx->join_ppp = (double)total / (double)no;
    if ((int64_t)total > cap || (total > 0 && !pairs)) return GF_ERR_CAPACITY;
    return GF_OK;
  }
  GF_HIP_CHECK(ctx, hipMemsetAsync(U32(o_hist), 0, bins * sizeof(uint32_t), s));
  GF_HIP_CHECK(ctx, launch_join_qkeys(s, qry->x, qry->y, nq, qgrid->minX, qgrid->minY, qgrid->cellLength,
                                      qgrid->n, U32(o_keys), I32(o_qcx), I32(o_qcy)));
  GF_HIP_CHECK(ctx, launch_histogram(s, U32(o_keys), nq, U32(o_hist)));
  GF_HIP_CHECK(ctx, launch_exclusive_scan(s, U32(o_hist), bins, U32(o_off), U32(o_tmp)));
  GF_HIP_CHECK(ctx, hipMemcpyAsync(U32(o_cur), U32(o_off), bins * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  GF_HIP_CHECK(ctx, launch_join_qscatter(s, qry->x, qry->y, I32(o_qcx), I32(o_qcy), U32(o_keys), nq, U32(o_cur),
                                         F64(o_sqx), F64(o_sqy), I32(o_sqcx), I32(o_sqcy), U32(o_sqi)));
  JoinArgs a{};
  a.ox = ord->x; a.oy = ord->y; a.no = no;
  a.u_minX = ugrid->minX; a.u_minY = ugrid->minY; a.u_cl = ugrid->cellLength;
  a.qn = qgrid->n; a.c = c; a.q_off = U32(o_off);
  a.sqx = F64(o_sqx); a.sqy = F64(o_sqy); a.sqcx = I32(o_sqcx); a.sqcy = I32(o_sqcy); a.sqidx = U32(o_sqi);
  a.approx = approximate != 0; a.metric = metric; a.r = r;
  a.counts = U32(o_cnt); a.offsets = U32(o_boff); a.pairs = pairs;
  GF_HIP_CHECK(ctx, launch_join_probe(ctx, a, 0, blocks));
  GF_HIP_CHECK(ctx, launch_exclusive_scan(s, U32(o_cnt), blocks, U32(o_boff), U32(o_tmp)));
  uint32_t total = 0;
  if (int e = read_scalar_sync(ctx, U32(o_boff) + blocks, &total)) return e;
  *npairs = total;
  if ((int64_t)total > cap) return GF_ERR_CAPACITY;
  if (total == 0) return GF_OK;
  if (!pairs) return set_err(ctx, GF_ERR_ARG, "null pairs");
  GF_HIP_CHECK(ctx, launch_join_probe(ctx, a, 1, blocks));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return GF_OK;
}

extern "C" int gf_join_pp(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* ord,
                          const gf_points* qry, double r, int approximate, int metric, uint32_t* pairs, int64_t cap,
                          int64_t* npairs) {
  return join_pp_impl(ctx, ugrid, qgrid, ord, qry, r, approximate, metric, pairs, cap, npairs, nullptr);
}

extern "C" int gf_join_pp_async(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* ord,
                                const gf_points* qry, double r, int approximate, int metric, uint32_t* pairs,
                                int64_t cap, unsigned long long* total) {
  if (!total) return set_err(ctx, GF_ERR_ARG, "gf_join_pp_async: null total");
  int64_t n = 0;
  int st = join_pp_impl(ctx, ugrid, qgrid, ord, qry, r, approximate, metric, pairs, cap, &n, total);
  if (st == GF_ERR_CAPACITY) st = GF_OK;  // the count is in *total
  if (st) return st;
  if (!ctx->join_async_done) {  // the synchronous paths (r == 0, empty sides): store the count
    const unsigned long long v = (unsigned long long)n;
    GF_HIP_CHECK(ctx, hipMemcpyAsync(total, &v, sizeof v, hipMemcpyHostToDevice, ctx->stream));
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GF_OK;
}

// the exact record of one window (any k, status 0), stream-ordered on the context stream
int gf::knn_exact_record(gf_knn_plan* P, const gf_points* pts, void* result) {
  int st = gf_knn_plan_flush(P);  // lane 0 is free afterwards
  if (st) return st;
  return knn_large(P, pts, result);
}

// ---------------------------------------------------------------------------------------
// windows, synthetic input
// ---------------------------------------------------------------------------------------
extern "C" int gf_pinned_alloc(size_t bytes, void** ptr) {
  if (!ptr || bytes == 0) return GF_ERR_ARG;
  *ptr = nullptr;
  // mapped + portable: the same pointer is written by kernels and read by the host
  hipError_t e = hipHostMalloc(ptr, bytes, hipHostMallocMapped | hipHostMallocPortable);
  if (e != hipSuccess) return GF_ERR_NOMEM;
  void* dptr = nullptr;
  if (hipHostGetDevicePointer(&dptr, *ptr, 0) != hipSuccess || dptr != *ptr) {
    hipHostFree(*ptr);
    *ptr = nullptr;
    return GF_ERR_HIP;  // unified addressing expected on gfx950
  }
  return GF_OK;
}

extern "C" void gf_pinned_free(void* ptr) {
  if (ptr) hipHostFree(ptr);
}

extern "C" int gf_window_create(gf_ctx* ctx, int64_t capacity, gf_window** out) {
  if (!ctx || !out || capacity < 0) return GF_ERR_ARG;
  int st = bind(ctx);
  if (st) return st;
  gf_window* w = new gf_window();
  w->ctx = ctx;
  w->capacity = capacity;
  const size_t n = (size_t)std::max<int64_t>(capacity, 1);
  if (hipMalloc(&w->x, 8 * n) != hipSuccess || hipMalloc(&w->y, 8 * n) != hipSuccess ||
      hipMalloc(&w->objID, 8 * n) != hipSuccess || hipMalloc(&w->ts, 8 * n) != hipSuccess ||
      hipStreamCreateWithFlags(&w->copy, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&w->ready, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&w->fence_main, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&w->fence_aux, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&w->fence_aux2, hipEventDisableTiming) != hipSuccess) {
    gf_window_destroy(w);
    return set_err(ctx, GF_ERR_NOMEM, "gf_window_create: device allocation failed");
  }
  *out = w;
  return GF_OK;
}

extern "C" void gf_window_destroy(gf_window* w) {
  if (!w) return;
  hipSetDevice(w->ctx->device);
  if (w->copy) hipStreamSynchronize(w->copy);
  hipStreamSynchronize(w->ctx->stream);
  sync_aux(w->ctx);
  if (w->x) hipFree(w->x);
  if (w->y) hipFree(w->y);
  if (w->objID) hipFree(w->objID);
  if (w->ts) hipFree(w->ts);
  if (w->ready) hipEventDestroy(w->ready);
  if (w->fence_main) hipEventDestroy(w->fence_main);
  if (w->fence_aux) hipEventDestroy(w->fence_aux);
  if (w->fence_aux2) hipEventDestroy(w->fence_aux2);
  if (w->copy) hipStreamDestroy(w->copy);
  delete w;
}

extern "C" int gf_window_upload(gf_window* w, const double* x, const double* y, const int64_t* objID,
                                const int64_t* ts, int64_t n) {
  if (!w || n < 0 || n > w->capacity || (n > 0 && (!x || !y))) return GF_ERR_ARG;
  gf_ctx* ctx = w->ctx;
  int st = bind(ctx);
  if (st) return st;
  // the copy waits for everything already enqueued on the context (evaluations of the old
  // contents), not for what is enqueued after this call
  GF_HIP_CHECK(ctx, hipEventRecord(w->fence_main, ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamWaitEvent(w->copy, w->fence_main, 0));
  if (ctx->aux) {
    GF_HIP_CHECK(ctx, hipEventRecord(w->fence_aux, ctx->aux));
    GF_HIP_CHECK(ctx, hipStreamWaitEvent(w->copy, w->fence_aux, 0));
  }
  if (ctx->aux2) {
    GF_HIP_CHECK(ctx, hipEventRecord(w->fence_aux2, ctx->aux2));
    GF_HIP_CHECK(ctx, hipStreamWaitEvent(w->copy, w->fence_aux2, 0));
  }
  const size_t b = 8 * (size_t)n;
  if (n) {  // only the columns given: range / join read x, y (16 B per point), kNN adds objID
    GF_HIP_CHECK(ctx, hipMemcpyAsync(w->x, x, b, hipMemcpyHostToDevice, w->copy));
    GF_HIP_CHECK(ctx, hipMemcpyAsync(w->y, y, b, hipMemcpyHostToDevice, w->copy));
    if (objID) GF_HIP_CHECK(ctx, hipMemcpyAsync(w->objID, objID, b, hipMemcpyHostToDevice, w->copy));
    if (ts) GF_HIP_CHECK(ctx, hipMemcpyAsync(w->ts, ts, b, hipMemcpyHostToDevice, w->copy));
  }
  GF_HIP_CHECK(ctx, hipEventRecord(w->ready, w->copy));
  w->has_objid = objID != nullptr;
  w->objid_mapped = nullptr;
  w->has_ts = ts != nullptr;
  w->pending = true;
  w->n = n;
  return GF_OK;
}

extern "C" int gf_host_pinned(const void* p, int* pinned) {
  if (!pinned) return GF_ERR_ARG;
  *pinned = 0;
  if (!p) return GF_OK;
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory is not a HIP allocation: clear the sticky error
    return GF_OK;
  }
  *pinned = at.type == hipMemoryTypeHost ? 1 : 0;
  return GF_OK;
}

extern "C" int gf_window_upload_mapped(gf_window* w, const double* x, const double* y, const int64_t* objID_pinned,
                                       int64_t n) {
  if (!w || (n > 0 && !objID_pinned)) return GF_ERR_ARG;
  void* dp = nullptr;
  if (n > 0) {  // the objID column is read in place through the host mapping (candidates only)
    int st = bind(w->ctx);
    if (st) return st;
    if (hipHostGetDevicePointer(&dp, (void*)objID_pinned, 0) != hipSuccess || !dp) {
      (void)hipGetLastError();  // clear the thread's sticky error: the next launch check must not see it
      return set_err(w->ctx, GF_ERR_ARG, "gf_window_upload_mapped: objID is not pinned host memory (gf_pinned_alloc)");
    }
  }
  int st = gf_window_upload(w, x, y, nullptr, nullptr, n);
  if (st) return st;
  w->objid_mapped = (const int64_t*)dp;
  return GF_OK;
}

extern "C" int gf_window_points(gf_window* w, gf_points* out) {
  if (!w || !out) return GF_ERR_ARG;
  if (w->pending) {  // work enqueued on the context from here on sees the uploaded contents
    gf_ctx* ctx = w->ctx;
    int st = bind(ctx);
    if (st) return st;
    GF_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, w->ready, 0));
    if ((st = gf_ctx_fork(ctx))) return st;  // a depth-3 plan may read the window from the second stream
    w->pending = false;
  }
  out->x = w->x; out->y = w->y; out->n = w->n;
  out->objID = w->objid_mapped ? w->objid_mapped : (w->has_objid ? w->objID : nullptr);
  out->ts = w->has_ts ? w->ts : nullptr;
  return GF_OK;
}

extern "C" int gf_synth_uniform(int64_t seed, int64_t n, double minX, double maxX, double minY, double maxY, double* x,
                                double* y) {
  if (n < 0 || (n > 0 && (!x || !y))) return GF_ERR_ARG;
  // java.util.Random: 48-bit LCG; nextDouble() = ((next(26) << 27) + next(27)) * 2^-53
  uint64_t sd = ((uint64_t)seed ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1);
  auto next = [&](int bits) {
    sd = (sd * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
    return (int64_t)(sd >> (48 - bits));
  };
  for (int64_t i = 0; i < n; ++i) {
    const double u = (double)((next(26) << 27) + next(27)) * 0x1.0p-53;
    x[i] = minX + u * (maxX - minX);
    const double v = (double)((next(26) << 27) + next(27)) * 0x1.0p-53;
    y[i] = minY + v * (maxY - minY);
  }
  return GF_OK;
}
