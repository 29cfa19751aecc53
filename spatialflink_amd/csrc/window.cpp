// window.cpp -- device-resident windows (upload on a copy stream of their own, ordered against the
// context's streams by events) and the synthetic input generator.
#define GF_TU_NAME window_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <algorithm>

#include "gf_internal.hpp"

using namespace gf;

// ---------------------------------------------------------------------------------------
// windows, synthetic input
// ---------------------------------------------------------------------------------------
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
