// The translation units of libgeoflink_hip.so: X(<stem>, <ext>) names the file <stem>.<ext> in this
// directory, whose GF_TU_NAME is <stem>_<ext> (gf_buildtag.hpp).  gf_build_info() and
// gf_build_is_product() (ctx.cpp) walk this list, so a unit missing from it could carry experiment
// defines unseen: tests/test_build_hygiene.py holds it, and the Makefile's SOURCES, equal to the
// directory's *.cpp / *.hip files.
#pragma once

#define GF_UNITS(X)                                                                            \
  X(ctx, cpp) X(grid, cpp) X(range, cpp) X(knn, cpp) X(join, cpp) X(window, cpp) X(comm, cpp)  \
  X(sliding, cpp) X(csv, cpp) X(objid, cpp) X(traj, cpp) X(tagg, cpp) X(tknn, cpp) X(tjoin, cpp) X(trange, cpp) X(geom, cpp) X(geomjoin, cpp) X(geomingest, cpp) X(wktingest, cpp) X(k_points, hip) X(k_knn, hip) \
  X(k_range, hip) X(k_join, hip) X(k_csv, hip) X(k_objid, hip) X(k_traj, hip) X(k_tagg, hip) \
  X(k_tknn, hip) X(k_tjoin, hip) X(k_trange, hip) X(k_geom, hip) X(k_geompair, hip) X(k_geomjoin, hip) X(k_geomingest, hip) X(k_wktingest, hip)
