// gf_geom_index.hpp -- the index of one geometry window (gf_geom_prepare, geom.cpp), for the host units
// that read it: geom.cpp (range and kNN against it) and geomjoin.cpp (two of them joined).
#pragma once

#include "gf_geom_plan.hpp"
#include "gf_group.hpp"

struct gf_geom_index {
  gf_ctx* ctx = nullptr;
  gf_grid grid{};
  gf_geoms geoms{};  // the window's device arrays (borrowed)
  int64_t nrings = 0;
  int32_t wide_vertices = gf::kGeomWideVertices;
  gf::DevArr<double> ring_env, env;
  gf::DevArr<uint8_t> ring_ok, valid;
  gf::DevArr<uint32_t> ring_wide, work_short, work_wide;
  gf::DevArr<int32_t> cells, nvert;
  gf::DevArr<unsigned long long> ctr;
};
