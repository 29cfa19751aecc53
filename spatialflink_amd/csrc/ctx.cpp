// ctx.cpp -- library and context entry points of the C ABI (include/geoflink_hip.h): errors,
// the context's scratch / pinned staging, the kernel timers, the look-back state of the single-pass
// scans, the build-info table, flags, streams, pinned host memory.
#define GF_TU_NAME ctx_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>

#include "gf_host.hpp"
#include "gf_units.hpp"

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

// Two kinds of event, two pools; an event of one kind is never handed out as the other.
//   timing    (KTimer): timestamps only.  Without the system-scope fence a record neither writes
//             back nor invalidates the caches under the launches around it.
//   ordering  (gf_ctx_join / gf_ctx_fork): order streams of this one device, so a device-scope
//             release is enough, and no timestamp is taken.
// Nothing read the host through either: records in mapped pinned memory are read after a stream
// or device synchronise, which releases to system scope itself.
static hipEvent_t take_event(std::vector<hipEvent_t>& pool, unsigned flags) {
  if (!pool.empty()) {
    hipEvent_t e = pool.back();
    pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  hipEventCreateWithFlags(&e, flags);
  return e;
}
static hipEvent_t take_timing_event(gf_ctx* ctx) { return take_event(ctx->pool, hipEventDisableSystemFence); }
static hipEvent_t take_order_event(gf_ctx* ctx) {
  return take_event(ctx->order_pool, hipEventDisableTiming | hipEventReleaseToDevice);
}

KTimer::KTimer(gf_ctx* c, int k) : ctx(c), kid(k) {
  if (!(ctx->timing & (1 << k))) return;
  if (ctx->timing_period > 1 && (ctx->timing_seq[k]++ % ctx->timing_period) != 0) return;
  a = take_timing_event(ctx);
  b = take_timing_event(ctx);
  hipEventRecord(a, ctx->stream);
}
KTimer::~KTimer() {
  if (!a) return;
  hipEventRecord(b, ctx->stream);
  ctx->pending.push_back({a, b, kid});
}

}  // namespace gf

using namespace gf;

// Ticket + epoch-tagged status words of the decoupled look-back kernels (expand_async, scan1)
// for a launch of `blocks` blocks; lookback_launch (gf_host.hpp) advances ctx->expand_base by the
// tickets the launch takes.
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

int gf::scan1(gf_ctx* ctx, uint32_t* in, int64_t L, uint32_t* out) {
  const int64_t blocks = scan1_blocks(L);
  return lookback_launch(ctx, blocks, blocks, "launch_scan1", [&](const ExpandState& es) {
    return launch_scan1(ctx->stream, in, L, out, nullptr, 0, 0, es);
  });
}

// ---------------------------------------------------------------------------------------
// library / context
// ---------------------------------------------------------------------------------------
extern "C" int gf_abi_version(void) { return GF_ABI_VERSION; }

namespace gf {  // one tag per translation unit (gf_buildtag.hpp), declared and listed from GF_UNITS
#define GF_UNIT_DECL(stem, ext) const char* build_tag_##stem##_##ext();
GF_UNITS(GF_UNIT_DECL)
#undef GF_UNIT_DECL
struct UnitTag {
  const char* unit;
  const char* (*tag)();
};
#define GF_UNIT_ROW(stem, ext) {#stem "." #ext, build_tag_##stem##_##ext},
static const UnitTag kUnitTags[] = {GF_UNITS(GF_UNIT_ROW)};
#undef GF_UNIT_ROW
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
  for (auto e : ctx->order_pool) hipEventDestroy(e);
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
    hipEvent_t ev = take_order_event(ctx);
    GF_HIP_CHECK(ctx, hipEventRecord(ev, a));
    GF_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, ev, 0));
    ctx->order_pool.push_back(ev);
  }
  return GF_OK;
}

extern "C" int gf_ctx_fork(gf_ctx* ctx) {
  if (!ctx) return GF_ERR_ARG;
  if (!ctx->aux) return GF_OK;
  int st = bind(ctx);
  if (st) return st;
  hipEvent_t ev = take_order_event(ctx);
  GF_HIP_CHECK(ctx, hipEventRecord(ev, ctx->stream));
  for (hipStream_t a : {ctx->aux, ctx->aux2})
    if (a) GF_HIP_CHECK(ctx, hipStreamWaitEvent(a, ev, 0));
  ctx->order_pool.push_back(ev);
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
