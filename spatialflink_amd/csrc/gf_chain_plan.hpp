// gf_chain_plan.hpp -- the pure host part of the linestring plans (range.cpp and knn.cpp upload what
// it builds): validation of a gf_linestrings set, each line's bbox (the vertex envelope,
// LineString.java: HelperClass.getBoundingBox) and the sub-chain envelopes -- every chain cut into
// runs of `run` consecutive segments, one envelope per run.  No device call and no context here, so a
// stand-alone host program (tests/native/chain_plan_main.cpp, built with the host sanitizers) can
// drive it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/geoflink_hip.h"

namespace gf {

struct ChainTables {
  std::vector<int32_t> vert_off;  // [nline + 1]
  std::vector<double> vx, vy;
  std::vector<double> bbox;       // [max(nline, 1) * 4] x1, y1, x2, y2 (vertex envelope)
  std::vector<int32_t> run_off;   // [nline + 1] runs per line (CSR)
  std::vector<double> run_env;    // [max(runs, 1) * 4] x1, y1, x2, y2 of the run's vertices
};

// false: a null array of a non-empty set, offsets that do not start at 0 or a line of fewer than 2
// vertices (the reference's LineString constructor leaves a null JTS object for those and fails later)
inline bool chain_valid(const gf_linestrings* ls) {
  if (!ls || ls->nline < 0) return false;
  if (ls->nline == 0) return true;
  if (!ls->vert_off || !ls->vx || !ls->vy || ls->vert_off[0] != 0) return false;
  for (int32_t l = 0; l < ls->nline; ++l)
    if (ls->vert_off[l + 1] - ls->vert_off[l] < 2) return false;
  return true;
}

// of a valid set; run >= 1 segments per run (segment i of a line joins its vertices i and i + 1, so
// run j of the line owns vertices [j * run, min((j + 1) * run, nseg)] -- neighbours share one)
inline void chain_build(const gf_linestrings& ls, int run, ChainTables& T) {
  const int32_t nl = ls.nline;
  const int32_t nv = nl > 0 ? ls.vert_off[nl] : 0;
  T.vert_off.assign(1, 0);
  if (nl > 0) T.vert_off.assign(ls.vert_off, ls.vert_off + nl + 1);
  T.vx.assign(ls.vx, ls.vx + nv);
  T.vy.assign(ls.vy, ls.vy + nv);
  if (T.vx.empty()) { T.vx.push_back(0.0); T.vy.push_back(0.0); }
  T.bbox.assign(4 * (size_t)std::max(nl, 1), 0.0);
  T.run_off.assign(1, 0);
  T.run_env.clear();
  auto envelope = [&](int32_t a, int32_t b, double* e) {  // vertices [a, b]
    double mnx = ls.vx[a], mxx = mnx, mny = ls.vy[a], mxy = mny;
    for (int32_t v = a + 1; v <= b; ++v) {
      mnx = std::min(mnx, ls.vx[v]); mxx = std::max(mxx, ls.vx[v]);
      mny = std::min(mny, ls.vy[v]); mxy = std::max(mxy, ls.vy[v]);
    }
    e[0] = mnx; e[1] = mny; e[2] = mxx; e[3] = mxy;
  };
  for (int32_t l = 0; l < nl; ++l) {
    const int32_t v0 = ls.vert_off[l], nseg = ls.vert_off[l + 1] - v0 - 1;
    envelope(v0, v0 + nseg, &T.bbox[4 * (size_t)l]);
    for (int32_t s = 0; s < nseg; s += run) {
      double e[4];
      envelope(v0 + s, v0 + std::min(s + run, nseg), e);
      T.run_env.insert(T.run_env.end(), e, e + 4);
    }
    T.run_off.push_back((int32_t)(T.run_env.size() / 4));
  }
  if (T.run_env.empty()) T.run_env.assign(4, 0.0);
}

}  // namespace gf
