// Test-only host build of the window path's fp64 numerics (spatialflink_amd/csrc/gf_numerics.hpp):
// the very functions the kernels run, compiled for the CPU so tests/test_numeric_edges.py can hold
// them to numpy / exact rational arithmetic on millions of inputs.  Not part of the product.
#include <cstdint>

#include "../../spatialflink_amd/csrc/gf_numerics.hpp"

extern "C" {

void core_hypot_many(const double* x, const double* y, int64_t n, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = gf::fdlibm_hypot(x[i], y[i]);
}

void core_smax_many(const double* T, int64_t n, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = gf::smax_for(T[i]);
}

void core_s_prefilter_many(const double* T, int64_t n, int metric, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = gf::s_prefilter(T[i], metric);
}

// the host branch of cell_index: jint(floor((v - mn) / cl))
void core_cell_div_many(const double* v, const double* mn, const double* cl, int64_t n, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = gf::cell_index(v[i], mn[i], cl[i]);
}

// the device branch's multiply-by-reciprocal with its guard band: decided[i] and, when set, the cell
void core_cell_fast_many(const double* v, const double* mn, const double* cl, int64_t n, int32_t* out,
                         uint8_t* decided) {
  for (int64_t i = 0; i < n; ++i) {
    double c;
    decided[i] = gf::cell_index_fast(v[i], mn[i], cl[i], &c) ? 1 : 0;
    out[i] = decided[i] ? (int32_t)c : 0;
  }
}

void core_jint_many(const double* v, int64_t n, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = gf::jint(v[i]);
}

void core_layers(double cl, double r, int32_t* g, int32_t* c) {
  *g = gf::guaranteed_layers(cl, r);
  *c = gf::candidate_layers(cl, r);
}

}  // extern "C"
