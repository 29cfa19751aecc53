// gf_host.hpp -- what the host units (*.cpp) share and no kernel unit needs: argument checks,
// the scratch arena, and the one home of each launch protocol the operators repeat.  The k_*.hip
// units include gf_internal.hpp only.
#pragma once

#include <algorithm>
#include <cassert>
#include <cmath>
#include <vector>

#include "gf_internal.hpp"

namespace gf {

// Several aligned buffers carved out of the context's scratch allocation: every take() names the
// pointer that receives its buffer, alloc() sizes the scratch and resolves them all.
struct Arena {
  size_t off = 0;
  template <class T>
  void take(T*& ptr, size_t count) {
    assert(nslots < kMaxSlots);
    const size_t o = (off + 255) & ~(size_t)255;
    off = o + count * sizeof(T);
    slots[nslots++] = {(void**)&ptr, o};
  }
  int alloc(gf_ctx* ctx) {
    int st = GF_OK;
    char* base = (char*)ctx_scratch(ctx, off, &st);
    if (st) return st;
    for (int i = 0; i < nslots; ++i) *slots[i].ptr = base + slots[i].off;
    return GF_OK;
  }

 private:
  static constexpr int kMaxSlots = 48;
  struct Slot { void** ptr; size_t off; };
  Slot slots[kMaxSlots];
  int nslots = 0;
};

// Launchers take ctx->stream: work for another stream swaps it in for a scope, and every exit
// from the scope puts the caller's stream back.
struct StreamScope {
  gf_ctx* ctx;
  hipStream_t saved;
  StreamScope(gf_ctx* c, hipStream_t s) : ctx(c), saved(c->stream) { c->stream = s; }
  ~StreamScope() { ctx->stream = saved; }
  StreamScope(const StreamScope&) = delete;
  StreamScope& operator=(const StreamScope&) = delete;
};

inline bool grid_ok(const gf_grid* g) {
  return g && g->n > 0 && std::isfinite(g->minX) && std::isfinite(g->minY) && std::isfinite(g->cellLength) &&
         g->cellLength > 0.0;
}

inline int check_points(gf_ctx* ctx, const gf_points* p) {
  if (!p || p->n < 0) return set_err(ctx, GF_ERR_ARG, "invalid gf_points");
  if (p->n > (int64_t)UINT32_MAX) return set_err(ctx, GF_ERR_ARG, "window larger than 2^32-1 points");
  if (p->n > 0 && (!p->x || !p->y)) return set_err(ctx, GF_ERR_ARG, "null x/y");
  if ((((uintptr_t)p->x) | ((uintptr_t)p->y)) & 15) return set_err(ctx, GF_ERR_ALIGN, "x/y must be 16-byte aligned");
  return GF_OK;
}

inline int stream_blocks(gf_ctx* ctx, int64_t items_per_thread_pairs) {
  int64_t b = (items_per_thread_pairs + kBlock - 1) / kBlock;
  const int64_t cap = (int64_t)ctx->num_cus * 8;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// One device scalar -> host through the pinned staging, then a stream sync (a pageable
// destination is copied by a staged blit, ~50 us per call in the join's rocprofv3 trace).
template <class T>
int read_scalar_sync(gf_ctx* ctx, const void* dev, T* out) {
  int st = GF_OK;
  T* h = (T*)ctx_pinned(ctx, sizeof(T), &st);
  if (!h) return st;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(h, dev, sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  *out = *h;
  return GF_OK;
}

// a plan's host table -> a device buffer of its own (plan creation: synchronous)
template <class T>
int upload(gf_ctx* ctx, T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  if (src.empty()) return GF_OK;
  GF_HIP_CHECK(ctx, hipMalloc(dst, src.size() * sizeof(T)));
  GF_HIP_CHECK(ctx, hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return GF_OK;
}

// exact cell thresholds (grid.cpp)
double first_at_least(int64_t A, double mn, double cl);
AxisIv axis_iv(int64_t a, int64_t b, double mn, double cl);
QueryRect make_qrect(const gf_grid& g, int32_t qcx, int32_t qcy, int32_t gl, int32_t cl);

// One launch of a decoupled look-back kernel (scan1, expand_async, the CSV newline index).  Its
// blocks take tickets [expand_base, expand_base + tickets) from the device counter, so the host's
// base must advance by exactly what the launch consumes, and only when it was issued: a base
// that runs ahead of (or behind) the device ticket leaves the next look-back kernel spinning on
// status words nobody writes.  `launch(es)` issues the kernel; this is the only place the base moves.
template <class Launch>
int lookback_launch(gf_ctx* ctx, int64_t blocks, int64_t tickets, const char* what, Launch launch) {
  ExpandState es;
  if (int st = lookback_state(ctx, blocks, &es)) return st;
  const hipError_t e = launch(es);
  if (e != hipSuccess) return hip_err(ctx, e, what);
  ctx->expand_base += (unsigned long long)tickets;
  return GF_OK;
}

// out[0 .. L] = exclusive scan of in[0 .. L) on the context stream, single pass (ctx.cpp)
int scan1(gf_ctx* ctx, uint32_t* in, int64_t L, uint32_t* out);

// grid of the radix passes over n keys: the scatter's tile buffers bound the blocks per CU
// (radix_threads), >= ~4 tiles per block
inline int radix_blocks(gf_ctx* ctx, int64_t n) {
  const int64_t tiles = (n + radix_tile() - 1) / radix_tile();
  return (int)std::min<int64_t>(std::max<int64_t>(tiles / 4, 1), (int64_t)radix_max_blocks(ctx->num_cus));
}

}  // namespace gf
