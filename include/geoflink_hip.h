/*
 * geoflink_hip.h -- C ABI of libgeoflink_hip.so, the MI355X (gfx950) window-evaluation
 * hot path of GeoFlink / SpatialFlink (reference: marianaGarcez/SpatialFlink).
 *
 * This is the drop-in boundary of BASELINE.json's north star: at each window trigger the
 * Java operators (UniformGrid, PointStream, RangeQuery, KNNQuery, JoinQuery) hand one
 * window's points across JNI as SoA buffers (x, y, objID, timestamp) and get the window's
 * result back.  Every entry point cites the reference code it replaces.  Plain C types only
 * (no torch, no C++); integer status codes, never exceptions or aborts across the boundary
 * (the reference's System.exit(1) becomes GF_ERR_LAYERS).  INTEGRATION.md shows the JNI
 * binding a maintainer adds on the Java side.
 *
 * Conventions
 *  - gf_points buffers are DEVICE pointers (HBM-resident windows).  x and y must be
 *    16-byte aligned (double2 loads).  gf_window_* upload host windows for callers that
 *    hold host buffers (JNI DirectByteBuffer / primitive arrays).
 *  - "async" calls only enqueue on the context's stream; "sync" calls return when results
 *    are on the host.
 *  - All arithmetic is IEEE binary64, round-to-nearest, no FMA contraction (Java never
 *    fuses), so cell IDs, range/join sets and kNN (objID, rank) lists match the reference
 *    restatement bit for bit.
 */
#ifndef GEOFLINK_HIP_H
#define GEOFLINK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF_ABI_VERSION 2

/* status codes */
#define GF_OK             0
#define GF_ERR_ARG       -1  /* invalid argument (reference: IllegalArgumentException) */
#define GF_ERR_CAPACITY  -2  /* output capacity too small; the required count is returned */
#define GF_ERR_HIP       -3  /* HIP runtime error (see gf_ctx_last_error) */
#define GF_ERR_NOMEM     -4
#define GF_ERR_LAYERS    -5  /* candidate layers <= 0 where the reference calls System.exit(1)
                                (UniformGrid.java:272-276, JoinQuery.java:80) */
#define GF_ERR_ALIGN     -7  /* x / y not 16-byte aligned */
#define GF_ERR_COMM      -8  /* RCCL unavailable or a collective failed (see gf_comm_last_error) */

/* distance metric of JTS Coordinate.distance */
#define GF_METRIC_SQRT  0    /* Math.sqrt(dx*dx + dy*dy) -- default */
#define GF_METRIC_HYPOT 1    /* Math.hypot(dx, dy) (fdlibm e_hypot) */

/* kernel ids for gf_ctx_timing */
#define GF_K_KNN_SCAN    0
#define GF_K_KNN_SAMPLE  1
#define GF_K_KNN_SELECT  2
#define GF_K_RANGE_SCAN  3
#define GF_K_ASSIGN      4
#define GF_K_JOIN_PROBE  5
#define GF_K_RANGE_TEST  6  /* point-polygon join passes (the range plans' deferred tests run in the scan) */
#define GF_K_JOIN_BUCKET 7  /* ordinary-side bucketing of the join */
#define GF_K_KNN_MERGE   8  /* top-k record merges (shards, sliding-window panes) */
#define GF_K_CSV_PARSE   9  /* CSV ingest: the per-line parse kernel */
#define GF_K_BUCKET      10 /* K2 bucketing by cell (gf_bucket_by_cell) */
#define GF_K_JOIN_COMPACT 11 /* join: packing of the probe's task regions */
#define GF_K_TRAJ_GROUP  12 /* trajectories: the group-by-objID kernels (its radix passes count as GF_K_BUCKET) */
#define GF_K_TSTATS      13 /* trajectories: tStats */
#define GF_K_TRAJ_SELECT 14 /* trajectories: sub-trajectory extraction */
#define GF_K_TAGG        15 /* tAggregate: its own kernels (the grouping kernels count as GF_K_TRAJ_GROUP, the radix passes as GF_K_BUCKET) */
#define GF_K_TKNN        16 /* tKnn: its own kernels (the grouping kernels count as GF_K_TRAJ_GROUP, the radix passes as GF_K_BUCKET) */
#define GF_K_TJOIN       17 /* tJoin: its own kernels (the radix passes count as GF_K_BUCKET) */
#define GF_K_TRANGE      18 /* tRange: the contains pass (gf_trange_points / gf_trange_run; the emit counts as GF_K_TRAJ_SELECT) */
#define GF_K_GEOM        19 /* polygon / linestring windows: prepare, classify and the exact passes (the kNN select counts as GF_K_KNN_SELECT) */
#define GF_K_COUNT       20

typedef struct gf_ctx gf_ctx;

/* UniformGrid(int n, minX, maxX, minY, maxY) -- UniformGrid.java:74-85 (value type) */
typedef struct {
  int32_t n;          /* numGridPartitions */
  int32_t reserved;
  double minX, maxX, minY, maxY;
  double cellLength;  /* (maxX - minX) / n, bounds NOT squared */
} gf_grid;

/* ---- objID keys ----------------------------------------------------------------------
 * The reference's objID is a String (Point.objID, Point.java:41-47; the CSV ingest keeps the
 * field as is, Deserialization.java:317 `String strOId`) and the kNN merge dedupes by
 * String.equals (KNNQuery.java:232-251).  gf_points.objID carries one int64 KEY per point,
 * injective over Strings:
 *   - a String that is exactly Long.toString(v) of a v in [-2^62, 2^62) -- "7", "-12"; not
 *     "007", "+7", " 7", "-0" -- has key v;
 *   - every other String has key INT64_MIN + id, its id in a gf_objid_dict -- assigned in first-
 *     occurrence order per batch, so keys never depend on scheduling.
 * Equal keys <=> equal Strings (keys of one dictionary).  The kNN contract's ties are broken by
 * key, so dictionary Strings order before numeric ones. */
#define GF_OBJID_NUMERIC_MIN (-(INT64_C(1) << 62))  /* keys below: dictionary Strings */
#define GF_OBJID_NUMERIC_END (INT64_C(1) << 62)     /* keys at or above: only GF_OBJID_NULL */
#define GF_OBJID_NULL INT64_MAX  /* a null objID (GeoJSON feature without the objID property) */
typedef struct gf_objid_dict gf_objid_dict;

/* One window of points as device SoA -- Point(objID, x, y, ts, uGrid), Point.java:91-100 */
typedef struct {
  const double* x;
  const double* y;
  const int64_t* objID;  /* objID keys (above); needed by kNN only */
  const int64_t* ts;     /* timeStampMillisec; read by the trajectory operators only */
  int64_t n;
} gf_points;

/* Query polygons (host CSR) -- Polygon(List<List<Coordinate>>, UniformGrid), Polygon.java:52-66.
 * Polygon p owns rings [ring_off[p], ring_off[p+1]); ring j owns vertices
 * [vert_off[j], vert_off[j+1]).  Ring 0 is the shell; rings are closed (first == last). */
typedef struct {
  int32_t npoly;
  const int32_t* ring_off;
  const int32_t* vert_off;
  const double* vx;
  const double* vy;
} gf_polygons;

/* Query linestrings (host CSR): line l owns vertices [vert_off[l], vert_off[l+1]), >= 2 each.  An
 * open chain: repeated vertices and first == last are legal and mean nothing special. */
typedef struct {
  int32_t nline;
  const int32_t* vert_off;
  const double* vx;
  const double* vy;
} gf_linestrings;

/* ---- library / context ------------------------------------------------------------- */
int         gf_abi_version(void);
/* Build identity (no reference counterpart): the compile-time tuning / experiment defines every
 * translation unit of this library was built with ("" per unit for the product build), and the
 * GF_* run-time knobs set in the environment.  gf_build_is_product() == 1 iff no unit carries a
 * command-line define -- the smoke and the GPU suite require it, so an experiment build
 * (tools/build_exp.sh) can never be measured or tested as the product. */
const char* gf_build_info(void);
int         gf_build_is_product(void);
const char* gf_status_string(int status);
int         gf_device_count(int* n);
/* One context per calling thread / Flink subtask; binds `device`, owns scratch + a stream. */
int         gf_ctx_create(int device, gf_ctx** out);
void        gf_ctx_destroy(gf_ctx* ctx);
/* Borrow a caller stream (hipStream_t), e.g. torch's current stream; NULL = the HIP null
 * stream.  A new context starts on its own non-blocking stream (returned by gf_ctx_stream). */
int         gf_ctx_set_stream(gf_ctx* ctx, void* hip_stream);
void*       gf_ctx_stream(gf_ctx* ctx);
int         gf_ctx_synchronize(gf_ctx* ctx);
/* Make the context stream wait for everything enqueued so far on the context's other streams
 * (kNN pipeline depth >= 3 launches windows there); no-op when it has none.  Host does not block. */
int         gf_ctx_join(gf_ctx* ctx);
/* The converse: make the other streams wait for everything enqueued so far on the context
 * stream.  Call it after producing a window on the context stream and before a depth >= 3
 * gf_knn_enqueue of it (gf_window_points and gf_knn_run do it themselves). */
int         gf_ctx_fork(gf_ctx* ctx);
const char* gf_ctx_last_error(gf_ctx* ctx);
/* Context flags (testing / tuning).  GF_FLAG_JOIN_LEGACY: 1 = gf_join_pp probes the query
 * buckets from global memory in input order instead of the row-bucketed LDS path.
 * GF_FLAG_JOIN_COARSE: 1 = the row-bucketed path never takes its sub-cell (fine) variant.
 * GF_FLAG_GEOJSON_WALK: 1 = gf_geojson_parse takes the member-by-member walk on every line
 * (no one-pass locator); the results are the same.
 * GF_FLAG_JOIN_STREAM: 1 = gf_join_pp's fine path buckets only the query side and streams the
 * ordinary points in input order (an experiment the default path is measured against).
 * GF_FLAG_GEOJSON_WAVE: 1 = gf_geojson_parse locates members with the wave-per-line structural
 * scan (r06, measured slower: DESIGN.md §3 GeoJSON) instead of one line per lane; same results.
 * GF_FLAG_GEOJSON_CHECK: 1 = gf_geojson_parse runs the wave scan AND the lane locator on every
 * staged line and counts their differences (gf_geojson_check_counts); results as the default. */
#define GF_FLAG_JOIN_LEGACY 1
#define GF_FLAG_JOIN_COARSE 2
#define GF_FLAG_GEOJSON_WALK 4
#define GF_FLAG_JOIN_STREAM 8
#define GF_FLAG_GEOJSON_WAVE 16
#define GF_FLAG_GEOJSON_CHECK 32
int gf_ctx_set_flag(gf_ctx* ctx, int flag, int value);
/* GF_FLAG_GEOJSON_CHECK's counts since the last read (then zeroed), after a sync: out[0] lines
 * both passed with the same member notes, out[1] the wave scan passed and the lane locator did not,
 * out[2] both passed with different notes, out[3] the lane locator passed and the wave scan did not
 * (a byte >= 0x80 sends a line to the walk).  out[1] and out[2] are defects. */
int gf_geojson_check_counts(gf_ctx* ctx, unsigned long long out[4]);

/* Record HIP events around launches of the kernels in `mask` (bit 1 << GF_K_*; 0 = off). */
int         gf_ctx_set_timing(gf_ctx* ctx, int mask);
/* Time only every period-th launch of each kernel (fewer events in a hot loop); default 1. */
int         gf_ctx_set_timing_period(gf_ctx* ctx, int period);
/* Sync, then return the summed kernel time (ms) and launch count for kernel_id; resets it. */
int         gf_ctx_timing(gf_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);

/* ---- grid / cell IDs (host) -------------------------------------------------------- */
int gf_grid_make(int32_t n, double minX, double maxX, double minY, double maxY, gf_grid* out);
/* getGuaranteedNeighboringLayers / getCandidateNeighboringLayers -- UniformGrid.java:428-445 */
int gf_grid_layers(const gf_grid* g, double r, int32_t* guaranteed, int32_t* candidate);
/* assignGridCellID(Coordinate) -- HelperClass.java:104-116 (host scalar form) */
int gf_cell_of(const gf_grid* g, double x, double y, int32_t* cx, int32_t* cy);
/* "%05d%05d" -- HelperClass.java:54-57,118-120; returns GF_ERR_CAPACITY if cap too small */
int gf_format_cell_id(int32_t cx, int32_t cy, char* buf, int32_t cap);
/* getIntCellIndices -- HelperClass.java:263-276 */
int gf_parse_cell_id(const char* id, int32_t* cx, int32_t* cy);

/* ---- K1: grid-cell assignment (async) -----------------------------------------------
 * Replaces HelperClass.assignGridCellID per point at ingest (Point.java:98).  cx/cy are
 * device int32[n]: cx = (int)Math.floor((x - minX)/cellLength), Java (int) saturation. */
int gf_assign_cells(gf_ctx* ctx, const gf_grid* g, const gf_points* pts, int32_t* cx, int32_t* cy);

/* ---- K2: bucketing by cell (async) -- the keyBy(gridID) shuffle (PointPointRangeQuery.java:144-148)
 * perm: device uint32[n], point indices grouped by cell; cell_start: device uint32[n*n + 2],
 * bucket b = valid cell cy*n + cx, bucket n*n = out-of-grid points: bucket b is
 * perm[cell_start[b] .. cell_start[b+1]).  Stable: inside a bucket the points keep their input
 * order (Flink's per-key window buffer iterates in arrival order), so the result is unique. */
int gf_bucket_by_cell(gf_ctx* ctx, const gf_grid* g, const gf_points* pts, uint32_t* perm,
                      uint32_t* cell_start);

/* ---- multi-GPU routing of an arriving window (async) ---------------------------------
 * The window's points partitioned by owning GPU: band b owns cell columns [band_lo[b],
 * band_lo[b+1]) (columns left of band_lo[1] -- out-of-grid ones too -- belong to band 0, those
 * right of the last start to the last band; NaN x counts as column 0).  perm: device
 * uint32[n], every band's points in arrival order; offsets: device uint32[nbands + 1], band b =
 * perm[offsets[b] .. offsets[b+1]).  One stable radix pass over the band keys (K1 + K2), the
 * keyBy(gridID) shuffle across ranks (PointPointRangeQuery.java:144-148).  nbands <= 64. */
int gf_shard_by_columns(gf_ctx* ctx, const gf_grid* g, const gf_points* pts, int32_t nbands, const int32_t* band_lo,
                        uint32_t* perm, uint32_t* offsets);
/* A band's SoA slice: out[i] = in[perm[begin + i]], i < end - begin, for the columns given
 * (device buffers; x, y, objID, ts may each be null). */
int gf_gather_points(gf_ctx* ctx, const gf_points* pts, const uint32_t* perm, int64_t begin, int64_t end, double* x,
                     double* y, int64_t* objID, int64_t* ts);

/* ---- range queries ----------------------------------------------------------------- */
typedef struct gf_range_plan gf_range_plan;
/* PointPointRangeQuery.run(stream, Set<Point> queryPoints, r) -- guaranteed / candidate cell
 * sets built once (PointPointRangeQuery.java:119-125); qx/qy host arrays. */
int  gf_range_pp_plan_create(gf_ctx* ctx, const gf_grid* g, const double* qx, const double* qy,
                             int32_t nq, double r, int approximate, int metric, gf_range_plan** out);
/* PointPolygonRangeQuery.run(stream, Set<Polygon>, r) -- PointPolygonRangeQuery.java:138-147 */
int  gf_range_ppoly_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_polygons* polys, double r,
                                int approximate, int metric, gf_range_plan** out);
void gf_range_plan_destroy(gf_range_plan* plan);
/* Window apply (PointPointRangeQuery.java:150-186 / PointPolygonRangeQuery.java:170-204), async.
 * bitmap: device uint64[(n+63)/64], bit i = point i emitted.  multi_bitmap (nullable): bit i =
 * point i emitted once per query point (approximate point-point, C cells).  counts: device
 * int64[2] = {points emitted, size of the emitted multiset}, summed by the last block of the
 * window's last kernel (no extra launch). */
int  gf_range_run(gf_range_plan* plan, const gf_points* pts, uint64_t* bitmap,
                  uint64_t* multi_bitmap, int64_t* counts);
/* Up to 16 windows of one plan in ONE launch (window w = pts[w], its bitmap bitmaps[w] and
 * counts[w] as gf_range_run; no multiplicity bitmap), plus -- idx non-null -- every window's
 * ascending index list in one more launch (idx[w] of capacity idx_cap[w], its length to
 * idx_count[w], as gf_bitmap_to_indices_async).  Async.  For windows that are available together
 * (a catch-up, several keys): small windows stop paying a launch each (PointPointRangeQuery.java:
 * 150-186 per window). */
int  gf_range_run_batch(gf_range_plan* plan, int32_t nwin, const gf_points* pts, uint64_t* const* bitmaps,
                        int64_t* const* counts, uint32_t* const* idx, const int64_t* idx_cap, int64_t* const* idx_count);
/* Plan diagnostics: in-grid cells by class (none / candidate / guaranteed / candidate cells
 * accepted untested because closed rectangles cover them); any pointer may be null. */
int  gf_range_plan_stats(const gf_range_plan* plan, int64_t* none_cells, int64_t* candidate_cells,
                         int64_t* guaranteed_cells, int64_t* inside_cells);
/* Tuning: scan blocks (0 = auto, <= 8 per CU); candidate tests: 0 auto, 1 inline in the scan,
 * 2 deferred (each scan block tests the candidate-cell points it queued at its end), 3 deferred
 * with the span prefilter (the scan only rules out points outside the class spans; every other
 * point is classified by the table at the block's end) -- table modes. */
int  gf_range_plan_set_tuning(gf_range_plan* plan, int32_t scan_blocks, int32_t defer_mode);
/* Testing: the deferred candidate tests at each scan block's end run on the first `lanes` lanes of
 * every wave only (1..64; 0 = all, the default).  Results are identical for any value: the drain
 * takes its points from a block cursor with whatever lanes are active (tests/test_gpu_parity.py). */
int  gf_range_plan_set_drain_lanes(gf_range_plan* plan, int32_t lanes);
/* Sync: selection bitmap -> ascending point indices (device uint32[cap]). */
int  gf_bitmap_to_indices(gf_ctx* ctx, const uint64_t* bitmap, int64_t n, uint32_t* idx,
                          int64_t cap, int64_t* count);
/* Async, one launch: the same indices (those past cap are not written) and their count into
 * device int64 *count -- enqueue it after gf_range_run so a window's step ends with the index
 * list the Java collector emits (PointPointRangeQuery.java:150-186) without a host sync. */
int  gf_bitmap_to_indices_async(gf_ctx* ctx, const uint64_t* bitmap, int64_t n, uint32_t* idx,
                                int64_t cap, int64_t* count);

/* ---- kNN ---------------------------------------------------------------------------- */
typedef struct gf_knn_plan gf_knn_plan;
/* PointPointKNNQuery.run(stream, queryPoint, r, k) -- PointPointKNNQuery.java:33,132-150 */
int    gf_knn_pp_plan_create(gf_ctx* ctx, const gf_grid* g, double qx, double qy, double r,
                             int32_t k, int metric, gf_knn_plan** out);   /* 1 <= k <= 2^24 */
/* k <= 512: sample -> scan -> one-block select (pipeline depths 1..3).  k > 512 (the
 * reference's PriorityQueue takes any k, KNNQuery.java:216): every candidate within r is kept
 * and the record comes from two stable device radix sorts of them ((objID, d, idx) -> first of
 * each objID -> (d, objID, idx)); the passes are sized by the window and bounded by the counts
 * on the device, so the enqueue never synchronizes and windows queue back to back at any
 * pipeline depth (each record complete in stream order); the sliding engine and
 * gf_knn_merge_dev(_batch) take records of any k.  The exact re-evaluation of a flagged window
 * (gf_knn_decode) takes the same sorted path. */
/* PointPolygonKNNQuery.run(stream, queryPolygon, r, k) -- knn/PointPolygonKNNQuery.java:245-317:
 * kNN of the window's points to ONE query polygon (polys->npoly == 1): candidates have their cell
 * in C u G of the polygon's bbox cells and d <= r, d = JTS point-polygon distance (0 inside) or,
 * approximate, DistanceFunctions.getPointPolygonBBoxMinEuclideanDistance.  Same records, decode
 * and contract as point queries ((d, objID) order, one entry per objID); pipeline depth <= 2. */
int    gf_knn_ppoly_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_polygons* polys, double r, int32_t k,
                                int approximate, int metric, gf_knn_plan** out);
void   gf_knn_plan_destroy(gf_knn_plan* plan);
/* Candidate-buffer capacity (entries); default 1<<20.  Small values force the exact fallback. */
int    gf_knn_plan_set_capacity(gf_knn_plan* plan, int64_t cap);
/* Scan-kernel tuning: grid blocks (0 = auto), point pairs per lane per iteration (1..8),
 * nontemporal loads (0/1).  Results never depend on it. */
int    gf_knn_plan_set_tuning(gf_knn_plan* plan, int32_t scan_blocks, int32_t unroll, int32_t nontemporal);
/* Continuous-query threshold hint (default on): each window stores 2 x its k-th distance and
 * the next window scans only below it (still verified: >= k distinct objIDs or re-evaluate). */
int    gf_knn_plan_set_hint(gf_knn_plan* plan, int enable);
/* Offset added to the window-local point index in results (a shard's first global index). */
int    gf_knn_plan_set_index_base(gf_knn_plan* plan, int64_t base);
/* Continuous-query pipeline.  depth 1 (default): each enqueue runs sample -> scan -> select,
 * stream-ordered.  depth 2 (k <= 256; larger k below): ONE fused launch per window -- blocks 1.. scan window i
 * with the threshold hint left by window i-2 (two device lanes), block 0 runs window i-1's
 * select meanwhile.  Window i's record is therefore written by the NEXT enqueue on the plan,
 * or by gf_knn_plan_flush (stream-ordered on the context stream).  No sample kernel: a cold
 * or failed hint flags the window (status 1, re-evaluated exactly by gf_knn_decode) and the
 * threshold adapts (shrinks after an overflow, doubles when fewer than k lie below it).
 * depth d = 3 or 4 (k <= 256): S = d - 1 streams (the context stream + S - 1 non-blocking ones);
 * window i launches on stream i % S, scans lane i % 2S and selects window i - S -- the previous
 * launch on the same stream -- in block 0, so S launches are in flight and every dependency stays
 * stream-ordered.  Polygon plans: the same, with each window's refine after its prefilter launch.
 * Window buffers must be complete before their enqueue: no cross-stream wait is inserted for them
 * (gf_ctx_fork after producing one on the context stream); gf_knn_plan_flush joins the other
 * streams back.  k in (256, 512] at depth >= 2: the select needs the standalone kernel's sort
 * area, so it is not fused: each window runs [sample] + scan + select on its lane, its record
 * complete in stream order; depth d >= 3 spreads windows over S streams, one lane each.  k > 512:
 * see above.  The sliding engine rejects depth > 2.  Results are identical at every depth. */
int    gf_knn_plan_set_pipeline(gf_knn_plan* plan, int depth);
int    gf_knn_plan_flush(gf_knn_plan* plan);
/* Result record: gf_knn_header followed by double dist[k], int64 objID[k], int64 idx[k]. */
typedef struct {
  int32_t status;        /* 0 = final; 1 = needs the exact fallback (see gf_knn_decode);
                            2 = a GF_MERGE_FOREIGN_KEYS merge met dictionary objID keys */
  int32_t n;             /* entries (<= k) */
  int32_t k;
  int32_t flags;
  int64_t candidates;    /* candidates appended by the scan */
  double threshold;      /* distance threshold the scan used */
} gf_knn_header;
size_t gf_knn_result_bytes(int32_t k);
/* Per-cell heaps + windowAll merge (PointPointKNNQuery.java:159-200, KNNQuery.java:213-272),
 * async: writes one result record into device memory `result`. */
int    gf_knn_enqueue(gf_knn_plan* plan, const gf_points* pts, void* result);
/* Sync: decode a host copy of the record; if it asks for the exact fallback, run it on pts.
 * Outputs sorted ascending by (dist, objID): rank = position. */
int    gf_knn_decode(gf_knn_plan* plan, const gf_points* pts, const void* result_host,
                     int64_t* objID, double* dist, int64_t* idx, int32_t* n_out);
/* Sync convenience: enqueue + copy + decode. */
int    gf_knn_run(gf_knn_plan* plan, const gf_points* pts, int64_t* objID, double* dist,
                  int64_t* idx, int32_t* n_out);
/* Merge per-shard top-k records (device, `nrec` <= 64 contiguous records of
 * gf_knn_result_bytes(k)) into one record (async) -- the windowAll funnel across GPUs after
 * an RCCL all-gather.  `result` may be device memory or gf_pinned_alloc memory.  Any k
 * (1 <= k <= 2^24): k <= 512 in one 256-thread block's LDS; larger k ranks every entry by binary
 * searches in the other records (each is sorted by (d, objID, idx)) and dedupes objIDs through
 * a hash table in the context's scratch, one 1024-thread block per window. */
int    gf_knn_merge_dev(gf_ctx* ctx, int32_t k, const void* records, int32_t nrec, void* result);
/* Batched: nwin windows in one launch (one block each), so one RCCL all-gather can carry the
 * records of several windows.  layout GF_MERGE_SHARD_MAJOR: record (shard s, window w) at
 * index s*nwin + w (an all-gather of each rank's nwin consecutive records);
 * GF_MERGE_WINDOW_MAJOR: at index w*nrec + s.  `results` receives nwin consecutive records.
 * layout | GF_MERGE_FOREIGN_KEYS: the records come from other contexts (an all-gather across
 * ranks).  Dictionary objID keys (below GF_OBJID_NUMERIC_MIN, GF_OBJID_NULL aside) are ids in
 * their own context's gf_objid_dict, so keys of different ranks cannot be compared or deduped:
 * a window holding one gets status 2 (GF_KNN_STATUS_FOREIGN_KEYS) and no entries -- merge such
 * windows by their Strings instead (gf_knn_attach_strings + gf_knn_merge_dev_strings below).
 * Canonical decimal objIDs are their values and merge across ranks. */
#define GF_MERGE_SHARD_MAJOR  0
#define GF_MERGE_WINDOW_MAJOR 1
#define GF_MERGE_FOREIGN_KEYS 0x100
#define GF_KNN_STATUS_FOREIGN_KEYS 2
int    gf_knn_merge_dev_batch(gf_ctx* ctx, int32_t k, const void* records, int32_t nrec, int32_t nwin,
                              int32_t layout, void* results);
/* ---- String objIDs across ranks (KNNQuery.java:232-251 dedupes by String.equals; MN_Q1.java:52
 * feeds gps.deviceId Strings).  A dictionary key is an id in its own rank's dictionary, so the
 * records travel with their Strings: a STRING RECORD is a kNN record followed by a sidecar
 * {int32 status, int32 n, int64 nbytes, uint32 off[k+1] (8-aligned), bytes[cap_bytes]} holding
 * the String of every dictionary objID of the record (entry i = bytes[off[i], off[i+1]), empty for
 * canonical decimal / null keys); sidecar status 1 = the Strings needed more than cap_bytes.
 *   rank r: gf_knn_attach_strings(its dictionary, its records) -> all-gather the string records
 *   -> gf_knn_merge_dev_strings on every rank -> the same merged string record everywhere.
 * The merge orders by (d, String, idx) -- dictionary Strings by their bytes (unsigned, a prefix
 * first) and before canonical decimals, decimals by value (null last) -- and keeps the first
 * entry of every String: rank independent.  (One rank's own select orders tied distances by
 * dictionary id; the cross-rank order differs from it only between different Strings at exactly
 * equal distances.)  The merged record's dictionary keys are the source ranks' and mean nothing
 * elsewhere: read its Strings with gf_knn_string_record_decode.  A flagged input record (status 1)
 * gives a flagged merged record (status 1, no entries: re-evaluate the shard exactly and exchange
 * again, as for gf_knn_exchange_batch); an input whose Strings did not fit its sidecar gives
 * status 2 (GF_KNN_STATUS_FOREIGN_KEYS, no entries: retry with a larger cap_bytes). */
size_t gf_knn_string_record_bytes(int32_t k, int64_t cap_bytes);
/* Async: nrec consecutive records (gf_knn_result_bytes(k) apart, device or pinned memory) ->
 * nrec consecutive string records (gf_knn_string_record_bytes(k, cap_bytes) apart) with the
 * Strings of their dictionary keys read from `dict` on the device. */
int gf_knn_attach_strings(gf_objid_dict* dict, int32_t k, const void* records, int32_t nrec, int64_t cap_bytes,
                          void* out);
/* Async: as gf_knn_merge_dev_batch (layouts, nrec <= 64, one block per window, any k) over string
 * records; results = nwin consecutive merged string records. */
int gf_knn_merge_dev_strings(gf_ctx* ctx, int32_t k, int64_t cap_bytes, const void* records, int32_t nrec,
                             int32_t nwin, int32_t layout, void* results);
/* Host: decode a host copy of a string record: *status (0 ok, else the record's / 2), entries
 * (objID keys, dist, idx; any may be null) and their Strings, String j = buf[offs[j], offs[j+1])
 * (Long.toString for canonical decimal keys, empty for null); GF_ERR_CAPACITY when buf_cap is too
 * small (offs[n] = the bytes needed). */
int gf_knn_string_record_decode(const void* record, int32_t k, int64_t cap_bytes, int32_t* status, int64_t* objID,
                                double* dist, int64_t* idx, char* buf, int64_t buf_cap, int64_t* offs, int32_t* n_out);
/* Host merge of per-shard sorted lists: top-k distinct objIDs by (dist, objID). */
int    gf_knn_merge_host(int32_t k, int32_t nlists, const int32_t* counts, const int64_t* objID,
                         const double* dist, const int64_t* idx, int64_t* out_objID,
                         double* out_dist, int64_t* out_idx, int32_t* n_out);

/* ---- multi-GPU: RCCL communicators and the kNN record exchange --------------------------------
 * The windowAll funnel across GPUs (PointPointKNNQuery.java:198-200 -> KNNQuery.java:213-272):
 * each GPU evaluates its cell-column band of the window (gf_shard_by_columns routes an arriving
 * window) into a top-k record; the exchange all-gathers every rank's records over xGMI (RCCL
 * ncclAllGather on the context's stream) and merges them on the device into the SAME record on
 * every rank (gf_knn_merge_dev_batch, shard-major; with > 1 rank GF_MERGE_FOREIGN_KEYS).  RCCL is
 * opened on first use (dlopen librccl.so.1; a process already holding it shares that copy).
 *   one process per GPU:  rank 0 gf_comm_unique_id -> broadcast the 128 bytes over the job's own
 *                         control plane -> every rank gf_comm_create(id, nranks, rank, device)
 *                         (ncclCommInitRank; blocks until all ranks joined);
 *   one process, N GPUs:  gf_comm_create_all(N, devices, comms) (ncclCommInitAll) -- then one
 *                         thread per GPU calls gf_knn_exchange_batch on its own comm, or one
 *                         thread drives all of them with gf_knn_exchange_group.
 * A communicator's exchanges must be enqueued on one stream (its gather buffer is reused in
 * stream order).  Every rank must call the exchange with the same k and nwin, in the same order.
 * Input records must be final (status 0): a flagged record (status 1) makes the merged record
 * flagged on every rank -- re-evaluate the shard exactly (gf_knn_decode) and exchange again. */
#define GF_COMM_ID_BYTES 128
typedef struct gf_comm gf_comm;
int  gf_comm_available(void);               /* 1 when librccl.so.1 loads and has every entry used */
int  gf_comm_unique_id(uint8_t* id);        /* id[GF_COMM_ID_BYTES] (ncclGetUniqueId), on one rank */
int  gf_comm_create(const uint8_t* id, int32_t nranks, int32_t rank, int device, gf_comm** out);
int  gf_comm_create_all(int32_t ndev, const int* devices, gf_comm** out /* [ndev] */);
void gf_comm_destroy(gf_comm* comm);        /* drains the device first */
int  gf_comm_info(const gf_comm* comm, int32_t* nranks, int32_t* rank, int* device);
const char* gf_comm_last_error(const gf_comm* comm);  /* comm == NULL: why this thread's last unique-id /
                                                      create call failed, else why RCCL did not load */
int  gf_comm_check(gf_comm* comm);          /* GF_ERR_COMM on an asynchronous RCCL error */
/* Async: this rank's nwin consecutive device records (gf_knn_result_bytes(k) apart; ctx's device
 * == the comm's) -> `merged` = nwin consecutive merged records (device or mapped pinned memory),
 * identical on every rank.  One all-gather + one merge launch for all nwin windows. */
int gf_knn_exchange_batch(gf_comm* comm, gf_ctx* ctx, int32_t k, const void* records, int32_t nwin, void* merged);
/* Async, String objIDs: the records' dictionary Strings attached from `dict` (on dict's context,
 * gf_knn_attach_strings), the string records all-gathered, merged by String
 * (gf_knn_merge_dev_strings) -> nwin merged string records (gf_knn_string_record_bytes apart). */
int gf_knn_exchange_strings_batch(gf_comm* comm, gf_objid_dict* dict, int32_t k, int64_t cap_bytes,
                                  const void* records, int32_t nwin, void* merged);
/* Async, one thread driving n communicators of one clique (gf_comm_create_all): the n
 * all-gathers as one RCCL group, then the n merges (comms[i] with ctxs[i], records[i], merged[i]).
 * comms must be the WHOLE clique (n == its size, each rank once; GF_ERR_ARG otherwise), checked
 * with every other argument before the group starts.  Should RCCL still fail inside the group,
 * the clique is aborted (ncclCommAbort: no all-gather is left waiting for a peer) and every later
 * call on those communicators returns GF_ERR_COMM; destroy them and create a new clique. */
int gf_knn_exchange_group(int32_t n, gf_comm* const* comms, gf_ctx* const* ctxs, int32_t k,
                          const void* const* records, int32_t nwin, void* const* merged);

/* ---- sliding-window kNN: pane engine ------------------------------------------------
 * PointPointKNNQuery.windowBased with SlidingProcessingTimeWindows.of(size, slide)
 * (PointPointKNNQuery.java:158,198-200; KNNQuery.java:213-272).  The reference re-evaluates
 * every window from scratch (each point size/slide times); here the stream is cut into panes
 * of gcd(size, slide) ms, each pane is evaluated ONCE on `plan` into a device record ring, and
 * a window's record is the top-k-distinct merge of its panes' records -- identical to
 * evaluating the window whole.  Pane p holds timestamps [p*pane_ms, (p+1)*pane_ms) (Flink
 * window assignment, offset 0); window [s, s + size), s a multiple of slide, closes with the
 * pane ending at s + size, and fires only if it holds a point.  Result idx = the point's position
 * in the pushed stream (panes concatenated in push order). */
typedef struct gf_knn_sliding gf_knn_sliding;
/* size / gcd(size, slide) <= 64; any k (k > 512: pane records from the sorted path, merged by
 * rank).  The plan's pipeline depth applies (depth 2: one fused launch per pane for k <= 256). */
int  gf_knn_sliding_create(gf_knn_plan* plan, int64_t size_ms, int64_t slide_ms, gf_knn_sliding** out);
void gf_knn_sliding_destroy(gf_knn_sliding* s);
/* pane length, panes per window / per slide, and how many of the latest panes the engine keeps
 * (their device buffers are borrowed and must stay valid while in the ring) */
int  gf_knn_sliding_geometry(const gf_knn_sliding* s, int64_t* pane_ms, int32_t* panes_per_window,
                             int32_t* panes_per_slide, int32_t* ring_panes);
/* Async.  Push pane `pane_index` (consecutive indices; an empty pane is pushed with n = 0).  If
 * a window closes with it, *closed = 1, *window_end = its end (ms), and its record is written
 * to window_result (device or gf_pinned_alloc memory) -- at depth 2 by the next push or flush. */
int  gf_knn_sliding_push(gf_knn_sliding* s, int64_t pane_index, const gf_points* pane, void* window_result,
                         int32_t* closed, int64_t* window_end);
int  gf_knn_sliding_flush(gf_knn_sliding* s);
/* Sync: decode a host copy of a window record; a flagged record (a pane needed the exact
 * fallback) is re-evaluated pane by pane (the panes must still be in the ring). */
int  gf_knn_sliding_decode(gf_knn_sliding* s, int64_t window_end, const void* result_host, int64_t* objID,
                           double* dist, int64_t* idx, int32_t* n_out);

/* ---- sliding range: the pane engine for PointPointRangeQuery / PointPolygonRangeQuery under
 * SlidingProcessingTimeWindows.of(size, slide) (PointPointRangeQuery.java:149-186,
 * PointPolygonRangeQuery.java:170-204).  Each pane (gcd(size, slide) ms, as gf_knn_sliding) is
 * evaluated ONCE on `plan` -- gf_range_run into a device pane bitmap, compacted on the device into
 * the pane's index list -- and a closed window's emitted points are its panes' lists
 * concatenated: identical to evaluating the window whole (each point's test is independent).
 * Window indices are window-local: positions in the window's panes concatenated in push order,
 * ascending, each emitted point once (approximate multi-query multiplicity: gf_range_run). */
typedef struct gf_range_sliding gf_range_sliding;
/* size / gcd(size, slide) <= 64; plan: gf_range_pp_plan_create / gf_range_ppoly_plan_create */
int  gf_range_sliding_create(gf_range_plan* plan, int64_t size_ms, int64_t slide_ms, gf_range_sliding** out);
void gf_range_sliding_destroy(gf_range_sliding* s);
int  gf_range_sliding_geometry(const gf_range_sliding* s, int64_t* pane_ms, int32_t* panes_per_window,
                               int32_t* panes_per_slide);
/* Async.  Push pane `pane_index` (consecutive indices; an empty pane with n = 0; the pane's
 * device points must stay valid until the context stream has passed this call).  If a window
 * closes with it and holds a point: *closed = 1, *window_end = its end (ms), *window_n = its
 * points, and the stream writes the window's index list to idx (device or pinned uint32[cap])
 * and its length to *count (device or pinned int64).  cap < *window_n: GF_ERR_CAPACITY with
 * nothing enqueued (push the same pane again with a larger idx). */
int  gf_range_sliding_push(gf_range_sliding* s, int64_t pane_index, const gf_points* pane, uint32_t* idx,
                           int64_t cap, int64_t* count, int32_t* closed, int64_t* window_end, int64_t* window_n);

/* Async window assembler for a batch in timestamp order (processing-time ingestion):
 * bounds (device int64[npanes + 1]) [j] = first i with ts[i] >= (first_pane + j) * pane_ms, so
 * pane first_pane + j is the slice [bounds[j], bounds[j+1]).  ts must be non-decreasing. */
int  gf_pane_bounds(gf_ctx* ctx, const int64_t* ts, int64_t n, int64_t pane_ms, int64_t first_pane, int32_t npanes,
                    int64_t* bounds);

/* ---- objID dictionaries ----------------------------------------------------------------
 * Device hash table + byte arena of the non-canonical objID Strings of a stream of windows.
 * gf_csv_parse uses the context's default dictionary (gf_ctx_objid_dict, owned by the
 * context); a JNI shim maps Point.objID Strings with gf_objid_intern and decodes result keys
 * (kNN objIDs) with gf_objid_decode.  Not thread-safe: one dictionary per calling thread. */
int  gf_objid_dict_create(gf_ctx* ctx, gf_objid_dict** out);
void gf_objid_dict_destroy(gf_objid_dict* d);
int  gf_ctx_objid_dict(gf_ctx* ctx, gf_objid_dict** out);
int  gf_objid_dict_size(const gf_objid_dict* d, int64_t* n);
/* Sync: keys of n host Strings, String i = bytes[offs[i], offs[i+1]) (offs: n+1 entries). */
int  gf_objid_intern(gf_objid_dict* d, const char* bytes, const int64_t* offs, int64_t n, int64_t* keys);
/* Sync: the Strings of n keys, String i = buf[offs[i], offs[i+1]) (offs: n+1 entries);
 * GF_ERR_CAPACITY when cap is too small (offs[n] = the bytes needed). */
int  gf_objid_decode(gf_objid_dict* d, const int64_t* keys, int64_t n, char* buf, int64_t cap, int64_t* offs);

/* ---- CSV / TSV ingest ----------------------------------------------------------------
 * Deserialization.CSVTSVToTSpatial(uGrid, dateFormat, delimiter, csvTsvSchemaAttr).map
 * (Deserialization.java:291-325) over a chunk of text lines, on the device.  Per line: '"'
 * removed, fields split on `delimiter` with the surrounding whitespace (split("\\s*" + delimiter
 * + "\\s*")), objID = the String field[objid_field] as its key (objID keys above; any String,
 * whitespace kept), ts = Long.valueOf(field[time_field]), x / y = Double.valueOf(...) correctly
 * rounded; with `grid`, the cell of Point(objID, x, y, ts, uGrid) (Point.java:98) as well.
 * Fields are read in the reference's order (objID, time, x, y): the first missing or
 * malformed one names the line's error. */
typedef struct {
  char delimiter;          /* ',' ';' '\t' ... (one character) */
  char reserved[3];
  int32_t objid_field;     /* csvTsvSchemaAttr.get(0) */
  int32_t time_field;      /* csvTsvSchemaAttr.get(1) */
  int32_t x_field;         /* csvTsvSchemaAttr.get(2) */
  int32_t y_field;         /* csvTsvSchemaAttr.get(3) */
} gf_csv_schema;
#define GF_CSV_OK              0
#define GF_CSV_NUMBER_FORMAT   1  /* Long.valueOf / Double.valueOf throw NumberFormatException */
#define GF_CSV_UNSUPPORTED     2  /* valid Java literal the device path does not take: hexadecimal, or
                                     > 19 significant digits within 1e-19 of a rounding boundary;
                                     or an objID field of 1 MiB or more */
#define GF_CSV_MISSING_FIELD   3  /* the reference's List.get throws IndexOutOfBoundsException */
#define GF_CSV_EMPTY_LINE      4  /* an empty line (a trailing newline at the end is fine) */
/* Sync.  text: device bytes [len], 16-byte aligned, complete lines separated by '\n' ("\r\n"
 * accepted; the last line may lack its '\n').  Outputs: device arrays of capacity cap (cx, cy
 * nullable, need grid).  *n_out = lines.  GF_ERR_CAPACITY if lines > cap (*n_out = lines);
 * GF_ERR_ARG on a bad line: *bad_line = its 0-based index, *bad_kind = GF_CSV_*. */
int gf_csv_parse(gf_ctx* ctx, const char* text, int64_t len, const gf_csv_schema* schema, const gf_grid* grid,
                 double* x, double* y, int64_t* objID, int64_t* ts, int32_t* cx, int32_t* cy, int64_t cap,
                 int64_t* n_out, int64_t* bad_line, int32_t* bad_kind);
/* As gf_csv_parse, objID keys from `dict` (NULL: the context's default dictionary). */
int gf_csv_parse_dict(gf_ctx* ctx, gf_objid_dict* dict, const char* text, int64_t len, const gf_csv_schema* schema,
                      const gf_grid* grid, double* x, double* y, int64_t* objID, int64_t* ts, int32_t* cx, int32_t* cy,
                      int64_t cap, int64_t* n_out, int64_t* bad_line, int32_t* bad_kind);

/* ---- GeoJSON ingest ------------------------------------------------------------------
 * Deserialization.GeoJSONToTSpatial(uGrid, dateFormat, propertyTimeStamp, propertyObjID).map
 * (Deserialization.java:149-211) over a chunk of lines, one JSON object per line: the ObjectNode
 * the map receives -- the Kafka record {"key":..,"value":..} (JSONKeyValueDeserializationSchema)
 * -- or, with value_lines = 1, the record's value itself (a Feature as
 * Serialization.PointToGeoJSONOutputSchema writes it).  Per line, in the map's order:
 *  - the record must be strict JSON as Jackson reads it (no NaN / Infinity, leading zeros,
 *    unescaped control bytes; UTF-8 checked structurally), else GF_CSV_MISSING_FIELD;
 *  - V = "value" (last duplicate wins, Jackson ObjectNode); missing / not an object:
 *    GF_CSV_MISSING_FIELD (the map's NullPointerException);
 *  - geometry = readGeoJSON(V) (jts-io-common 1.18.0 GeoJsonReader): V's "type" "Point" ->
 *    V's "coordinates"; on failure, and for "Feature" or a missing / non-string / unknown
 *    "type", the reference's catch branch readGeoJSON(V.geometry): "type" "Point" and
 *    "coordinates", else the line fails (GF_CSV_MISSING_FIELD; a non-number ordinate
 *    GF_CSV_NUMBER_FORMAT).  x, y = ordinates 0 and 1 (an integer literal is (double) of its
 *    long: "-0" -> 0.0);
 *  - from V's "properties" (absent or not an object: objID null, ts 0): ts from time_property
 *    -- date_format 0: Long.parseLong of the node's text (a JSON integer; anything else throws
 *    NumberFormatException: GF_CSV_NUMBER_FORMAT), date_format 1: the string value parsed as
 *    SimpleDateFormat("yyyy-MM-dd HH:mm:ss") (lenient field rollover) in a fixed UTC offset
 *    (tz_offset_minutes; DST not modelled), unparsable -> 0; objID from objid_property --
 *    node.toString() without '"': a string's content, an integer's digits ("-0" -> "0"),
 *    true / false / null as text; absent -> GF_OBJID_NULL.
 * GF_CSV_UNSUPPORTED (not restated, never guessed): geometry types other than Point (JTS builds
 * and validates them) and FeatureCollection; Point coordinates with fewer than two ordinates or
 * a non-number third; a number Jackson hands json-simple as text it cannot read back (a float
 * literal overflowing to Infinity, an integer literal outside long) anywhere on the line;
 * nesting deeper than 256; escapes in a taken string or in a member name of an object a value is
 * looked up in; non-integer or structured objID values; years before 1583 (Julian calendar). */
typedef struct {
  const char* objid_property;   /* propertyObjID (host C string, < 64 bytes); NULL: objID always null */
  const char* time_property;    /* propertyTimeStamp; NULL: ts always 0 */
  int32_t date_format;          /* 0: integer milliseconds; 1: "yyyy-MM-dd HH:mm:ss" */
  int32_t tz_offset_minutes;    /* date_format 1: offset of the reference JVM's default zone */
  int32_t value_lines;          /* 0: each line is the record {"key":..,"value":..}; 1: its value */
} gf_geojson_schema;
/* Same conventions as gf_csv_parse_dict (device text, outputs, capacity, first bad line). */
int gf_geojson_parse(gf_ctx* ctx, gf_objid_dict* dict, const char* text, int64_t len, const gf_geojson_schema* schema,
                     const gf_grid* grid, double* x, double* y, int64_t* objID, int64_t* ts, int32_t* cx,
                     int32_t* cy, int64_t cap, int64_t* n_out, int64_t* bad_line, int32_t* bad_kind);

/* ---- GeoJSON ingest of polygon and linestring streams -----------------------------------
 * Deserialization.GeoJSONToSpatialPolygon / GeoJSONToTSpatialPolygon (Deserialization.java:327-458)
 * and GeoJSONToSpatialLineString / GeoJSONToTSpatialLineString (:623-745) over a chunk of lines:
 * text in, a geometry window (gf_geoms, below) out, on the device, ready for gf_geom_prepare.
 *
 * Shared with gf_geojson_parse (same code): the line is the Kafka record or, with value_lines, its
 * value V; strict JSON as Jackson reads it; V missing or not an object: GF_CSV_MISSING_FIELD; the
 * number rule (correctly rounded; an integral literal is (double) of its long, "-0" -> +0.0; a
 * float overflowing to Infinity or an integer outside long anywhere on the line: unsupported);
 * "properties" (time property, objID property, date_format, tz_offset_minutes, escapes, objID
 * keys through the dictionary); CRLF, a missing final newline, empty lines (GF_CSV_EMPTY_LINE),
 * nesting deeper than 256; the first bad line wins (GF_ERR_ARG, *bad_line, *bad_kind).  The non-T
 * deserializers are this call with both property names NULL: objID null, ts 0.
 *
 * Which geometry is taken (the maps' try / catch, :346-355, :641-650): V's own "type" names a
 * geometry -> V's "coordinates"; on failure, or for "Feature" / a missing / unknown "type" ->
 * V."geometry".  FeatureCollection: unsupported.  The taken geometry's "type" must be "Polygon" or
 * "MultiPolygon" (kind GF_GEOM_POLYGON), "LineString" or "MultiLineString" (GF_GEOM_LINESTRING);
 * any other GeoJSON geometry type is GF_CSV_UNSUPPORTED (the reference pushes it through the wrong
 * bracket depth).
 *
 * What JTS must accept (GeoJsonReader builds the geometry first; the kinds are this library's
 * labels, the reference only throws):
 *  - every position is an array whose ordinates 0 and 1 are numbers, else GF_CSV_NUMBER_FORMAT;
 *  - a non-array where a position, ring or polygon array is expected: GF_CSV_MISSING_FIELD;
 *  - every ring of a Polygon, and of every polygon of a MultiPolygon, has at least 4 positions and
 *    first == last (Coordinate.equals2D: x == x and y == y of the parsed doubles, so -0.0 closes
 *    0.0), else GF_CSV_MISSING_FIELD;
 *  - every linestring, every member of a MultiLineString included, has at least 2 positions, else
 *    GF_CSV_MISSING_FIELD.
 * Within one geometry the first failure in document order is the line's; ring closure is tested
 * after the structure of the whole geometry.
 *
 * The coordinates the object gets.  The reference re-reads V.toString() with a string splitter
 * (convertCoordinates / convertMultiCoordinates / splitString / findCountN, :1382-1427, :1531-1592)
 * that starts at the text's first '[', counts bracket depth and splits on "],".  On Jackson's
 * compact re-serialisation that equals the plain structural reading of the taken "coordinates"
 * exactly under these conditions; everything else is GF_CSV_UNSUPPORTED, never guessed:
 *  - no '[' or ']' byte in V's text before the '[' of the taken "coordinates" (a bbox, an
 *    array-valued property, a bracket inside a string); nor a backslash there (an escape can spell
 *    a bracket that the re-serialisation writes out).  Anything after the array is free;
 *  - every position has exactly two ordinates (a third stops the splitter from closing rings);
 *  - no empty array at any level of the taken "coordinates";
 *  - no duplicate member name in V or in the taken geometry object (Jackson keeps the first
 *    position and the last value);
 *  - if V's own geometry fails and the catch branch's "geometry" succeeds, the splitter still
 *    reads V's first bracket: unsupported.
 *
 * The window object (what the operators read: .polygon, .lineString):
 *  - Polygon: its rings in createPolygon order (Polygon.java:147-165): one ring as is; several by
 *    descending area with the insertion rule of createPolygonArray (:115-145: appended while the
 *    last ring's area >= its own -- equal areas keep input order --, else inserted before the
 *    first ring whose area <= its own), the largest the shell.  The area is the plain shoelace
 *    sum x1*y2 - x2*y1 in ring order, fp64, no contraction, abs / 2 -- the one spatialObjects.Polygon
 *    uses, so the window is bit-identical to that host mirror's.  JTS's own getArea is believed to
 *    use an x-shifted form (not verifiable without JTS): rings whose order differs between the two
 *    forms, and rings whose area is not a number, are outside the contract.  Closing and padding
 *    never trigger: JTS has required closed rings of at least 4 positions.
 *  - MultiPolygon: its FIRST polygon only (MultiPolygon.java:32-45); the later ones are validated
 *    and dropped.  LineString: its positions.  MultiLineString: its FIRST linestring
 *    (MultiLineString.java:30-50).
 *  - objID and ts from "properties" as for points.
 *
 * The call is synchronous; text is device bytes, 16-byte aligned, shorter than 8 GiB.  On success
 * *nobj / *nrings / *nverts are exact and the arrays form a valid gf_geoms: offsets start at 0 and
 * are monotone, ring_off[nobj] == nrings, vert_off[last] == nverts (linestrings: *nrings = 0).
 * If any capacity is too small: GF_ERR_CAPACITY with all three exact counts and nothing promised
 * about the arrays; all capacities 0 with NULL arrays is the legal way to ask for the sizes.
 * Totals that do not fit int32 offsets: GF_ERR_ARG.  Argument errors are reported before any
 * device call.  Not restated here: CSV/TSV geometry lines, MultiPoint and GeometryCollection
 * streams (WKT lines: gf_wkt_parse_geoms, below). */
typedef struct {            /* device arrays the parse fills; capacities in elements */
  int32_t kind;             /* GF_GEOM_POLYGON | GF_GEOM_LINESTRING: which stream constructor */
  int64_t obj_cap, ring_cap, vert_cap;
  int32_t* ring_off;        /* [obj_cap + 1]; polygons only (NULL for linestrings) */
  int32_t* vert_off;        /* polygons [ring_cap + 1]; linestrings [obj_cap + 1] */
  double *vx, *vy;          /* [vert_cap] */
  int64_t *objID, *ts;      /* [obj_cap] */
} gf_geoms_out;
int gf_geojson_parse_geoms(gf_ctx* ctx, gf_objid_dict* dict /* NULL: the context's */, const char* text, int64_t len,
                           const gf_geojson_schema* schema, const gf_geoms_out* out, int64_t* nobj, int64_t* nrings,
                           int64_t* nverts, int64_t* bad_line, int32_t* bad_kind);

/* ---- WKT ingest of point, polygon and linestring streams -----------------------------------
 * Deserialization.WKTToSpatial / WKTToTSpatial (Deserialization.java:214-232, :261-288),
 * WKTToSpatialPolygon / WKTToTSpatialPolygon (:461-490, :524-586) and WKTToSpatialLineString /
 * WKTToTSpatialLineString (:748-835) with their WKTReader helpers (:1456-1528), over a chunk of
 * lines on the device.  Per line:
 *
 * Which text is read.  The geometry text starts at the first byte-exact, case-sensitive occurrence
 * of the tag, as String.indexOf finds it: polygons "MULTIPOLYGON" if it occurs, else "POLYGON";
 * linestrings "MULTILINESTRING" if it occurs, else "LINESTRING"; points "POINT".  No occurrence
 * (a lower-case tag included): the reference's substring(-1) throws, GF_CSV_MISSING_FIELD.  The
 * occurrence is taken where it is found -- inside a longer word, inside the line's first field --
 * and the grammar below decides.  Everything after the geometry's closing ')' is free (a T line's
 * time field, a closing quote, the "} of a Kafka record).
 *
 * The canonical grammar; every other text is GF_CSV_UNSUPPORTED or a failure where any WKT reader
 * must fail, never guessed: the tag, optional blanks (space or tab), '('; parentheses nested to the
 * depth the tag implies; members separated by ',' with optional blanks around them; a position is
 * exactly two number tokens separated by blanks; a number token is a maximal run of the bytes
 * 0-9 + - . e E and its value is Double.parseDouble of the token, correctly rounded.
 *  - GF_CSV_UNSUPPORTED: anything but blanks between the tag and its '(' (Z, M, ZM, EMPTY, a tag
 *    run-on such as POLYGONZ); EMPTY anywhere; a third number in a position; a token holding any
 *    other letter (NaN, Infinity, a d / f suffix, hexadecimal); '#', a byte >= 0x80 or a control
 *    byte other than tab inside the geometry text; a literal of more than 19 significant digits
 *    within 1e-19 of a rounding boundary (as GF_CSV_UNSUPPORTED of gf_csv_parse); a line of 2 GiB;
 *  - GF_CSV_NUMBER_FORMAT: a token of the allowed bytes that parseDouble rejects (1.2.3, -, e5);
 *  - GF_CSV_MISSING_FIELD (this library's label; the reference only throws): a position with one
 *    number, a line that ends before the geometry closes, a wrong bracket, an empty member list.
 *
 * What JTS must accept: every ring of the polygon (of every polygon of a MULTIPOLYGON) has at least
 * 4 positions and is closed under Coordinate.equals2D on the parsed doubles; every linestring, every
 * MULTILINESTRING member included, has at least 2 positions; else GF_CSV_MISSING_FIELD.  The first
 * failure in document order is the line's; ring closure is tested after the structure of the whole
 * geometry.
 *
 * The window object.  Polygon: exterior then interiors as getPolygonCoordinates lists them, then the
 * createPolygon order -- the same code and the same shoelace area as gf_geojson_parse_geoms.
 * MULTIPOLYGON: its first polygon only (the later ones are validated and dropped).  LINESTRING: its
 * positions.  MULTILINESTRING: its first member.  POINT: x and y of the one position, with cx, cy
 * when a grid is given.
 *
 * objID and ts (the T variants: delimiter != 0).  The line with every '"' removed is split by
 * gf_csv_parse's "\\s*delimiter\\s*" rule.  objID = field 0 after Java trim(), or null when the
 * trimmed field starts with one of the stream's two tags; it becomes a key as in gf_csv_parse_dict
 * (a canonical decimal is its value, any other String goes through the dictionary).  ts:
 * date_format 0 -> 0; date_format 1 -> the fields from the last to the first, each trimmed, through
 * gf_geojson_parse's date parser (SimpleDateFormat.parse reads a prefix), the first that parses; none
 * -> 0; a date before 1583 in a tried field: GF_CSV_UNSUPPORTED.  The reference's quirk (:577-582) is
 * kept: a POLYGON whose ts is 0 (a date that parses to the epoch included) is built by
 * Polygon(list, uGrid), so its objID is null; a MULTIPOLYGON and both linestring kinds keep their
 * objID at ts 0.  The fields are read before the geometry, as the maps do.  The non-T maps
 * (delimiter 0) read no field: objID null, ts 0.
 *
 * gf_wkt_parse_geoms follows every convention of gf_geojson_parse_geoms (gf_geoms_out and its kind;
 * device text, 16-byte aligned, shorter than 8 GiB; CRLF, a missing final newline; an empty line is
 * GF_CSV_EMPTY_LINE; all-zero capacities with NULL arrays is the sizing call; GF_ERR_CAPACITY returns
 * the three exact counts; the first bad line wins with GF_ERR_ARG, *bad_line, *bad_kind; argument
 * errors before any device call; totals past int32 offsets are GF_ERR_ARG; len == 0 is a valid empty
 * window).  gf_wkt_parse_points follows gf_csv_parse (outputs, capacity rule, bad-line report); both
 * point maps build Point(x, y, uGrid) -- the T variant ignores its date format and delimiter -- so
 * objID is GF_OBJID_NULL and ts 0 on every line, and the call takes no schema.
 * Rests on JTS 1.16.1 (not verifiable without it): WKTReader.read stops after the first
 * geometry; the tokenizer's character classes; the LinearRing / LineString size and closure checks;
 * no normalisation; getCoordinates in text order. */
typedef struct {
  char delimiter;            /* T variants: one character, as gf_csv_schema.delimiter: any byte is taken as
                                is and matched literally (not as a regex), except '"', which is GF_ERR_ARG:
                                every '"' is removed before the split, so it could never split;
                                0: the non-T deserializers (objID null, ts 0, no field is read) */
  char reserved[3];
  int32_t date_format;       /* 0: dateFormat == null (ts 0); 1: "yyyy-MM-dd HH:mm:ss" */
  int32_t tz_offset_minutes; /* as gf_geojson_schema */
} gf_wkt_schema;
int gf_wkt_parse_geoms(gf_ctx* ctx, gf_objid_dict* dict /* NULL: the context's */, const char* text, int64_t len,
                       const gf_wkt_schema* schema, const gf_geoms_out* out, int64_t* nobj, int64_t* nrings,
                       int64_t* nverts, int64_t* bad_line, int32_t* bad_kind);
int gf_wkt_parse_points(gf_ctx* ctx, const char* text, int64_t len, const gf_grid* grid, double* x, double* y,
                        int64_t* objID, int64_t* ts, int32_t* cx, int32_t* cy, int64_t cap, int64_t* n_out,
                        int64_t* bad_line, int32_t* bad_kind);

/* ---- join (sync) --------------------------------------------------------------------
 * JoinQuery.getReplicatedPointQueryStream + PointPointJoinQuery.windowBased
 * (JoinQuery.java:73-90, PointPointJoinQuery.java:124-183).  pairs: device uint32[2*cap]
 * (ordinary idx, query idx), unordered.  *npairs = pairs found; GF_ERR_CAPACITY (with *npairs =
 * the exact count) if and only if that count > cap: the window's output regions are sized from
 * the context's previous join, and the pairs of a block that outgrows its region go to a device
 * spill sized so that every window whose pairs fit cap completes in one call. */
int gf_join_pp(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* ordinary,
               const gf_points* query, double r, int approximate, int metric, uint32_t* pairs,
               int64_t cap, int64_t* npairs);
/* The same window join without a host wait: every launch stream-ordered on the context stream,
 * the pair count written by the last kernel to *total (device or mapped pinned memory), so the
 * next window's launches queue behind this one.  Pairs past cap are not written: the caller
 * re-runs the window with a larger buffer when *total > cap (*total = the exact count).  (r == 0
 * -- every cell a key --
 * takes the synchronous path and then stores *total.) */
int gf_join_pp_async(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* ordinary,
                     const gf_points* query, double r, int approximate, int metric, uint32_t* pairs,
                     int64_t cap, unsigned long long* total);

/* Point-polygon window join: JoinQuery.getReplicatedPolygonQueryStream + PointPolygonJoinQuery
 * .windowBased (JoinQuery.java:93-115, PointPolygonJoinQuery.java:154-213).  Polygon q is
 * replicated to its own G_q u C_q keys (UniformGrid.java:193-206,399-411) on qgrid; point p
 * (key on ugrid, which must equal qgrid here) pairs with q if approximate or the JTS distance
 * (DistanceFunctions.java:33-36) is <= r.  The plan is the replicated polygon side (reusable
 * while the polygon set is unchanged); gf_range_plan_destroy frees it.  Run (sync): pairs =
 * device uint32[2*cap] (point idx, polygon idx), unordered; *npairs = pairs found,
 * GF_ERR_CAPACITY if > cap (pairs may be null with cap 0 to count). */
int gf_join_ppoly_plan_create(gf_ctx* ctx, const gf_grid* qgrid, const gf_polygons* polys, double r,
                              int approximate, int metric, gf_range_plan** out);
int gf_join_ppoly_run(gf_range_plan* plan, const gf_grid* ugrid, const gf_points* points, uint32_t* pairs,
                      int64_t cap, int64_t* npairs);
/* One-shot: plan create + run + destroy (a polygon stream's window). */
int gf_join_ppoly(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* points,
                  const gf_polygons* polys, double r, int approximate, int metric, uint32_t* pairs,
                  int64_t cap, int64_t* npairs);

/* ---- query linestrings over point windows -----------------------------------------------
 * PointLineStringRangeQuery (range/PointLineStringRangeQuery.java:100-172),
 * PointLineStringKNNQuery (knn/PointLineStringKNNQuery.java, windowBased) and
 * PointLineStringJoinQuery (join/PointLineStringJoinQuery.java, windowBased): the point-polygon
 * window paths with the geometry renamed -- the cell sets come from the line's bbox cells
 * (UniformGrid.java:208-222, 413-426; JoinQuery.java:117-137), the approximate distance is the bbox
 * distance (DistanceFunctions.java:203-255) -- and one other exact distance: Point.distance(LineString)
 * (DistanceFunctions.java:38-42) is the minimum of Distance.pointToSegment over the open chain, with
 * no containment step (a point inside a closed chain is at its distance to the nearest segment).
 * The plans are ordinary gf_range_plan / gf_knn_plan objects: gf_range_run, gf_range_run_batch,
 * gf_range_plan_stats, the tuning calls, gf_range_sliding_*, gf_join_ppoly_run (the pair list's
 * second column is then the line index), gf_knn_enqueue / decode / run (pipeline depth <= 2 as for
 * polygon plans), gf_knn_sliding_* and the merges take them unchanged.  Errors as the polygon
 * creators: null or negative counts, a bad metric or a line of < 2 vertices -> GF_ERR_ARG; kNN takes
 * exactly one line; an empty set is a valid plan that matches nothing. */
int gf_range_pls_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_linestrings* lines, double r,
                             int approximate, int metric, gf_range_plan** out);
int gf_knn_pls_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_linestrings* lines /* nline == 1 */, double r,
                           int32_t k, int approximate, int metric, gf_knn_plan** out);
int gf_join_pls_plan_create(gf_ctx* ctx, const gf_grid* qgrid, const gf_linestrings* lines, double r,
                            int approximate, int metric, gf_range_plan** out);
int gf_join_pls(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* points,
                const gf_linestrings* lines, double r, int approximate, int metric, uint32_t* pairs,
                int64_t cap, int64_t* npairs);
/* Testing / tuning of a linestring plan's exact distance: 0 = chains longer than one run of segments
 * skip the runs whose envelope is provably farther than the bound (default), 1 = the plain segment
 * loop.  Results never depend on it.  GF_ERR_ARG for another mode or a plan that is no linestring plan. */
int gf_range_plan_set_chain_mode(gf_range_plan* plan, int mode);
int gf_knn_plan_set_chain_mode(gf_knn_plan* plan, int mode);

/* ---- trajectories -----------------------------------------------------------------------
 * The reference's t* operators (TStatsQuery, PointPolygonTRangeQuery, PointPointTKNNQuery, ...)
 * treat a window as a set of TRAJECTORIES: the points of one objID in arrival order
 * (keyBy(objID), then `for (Point p : input)`, TStatsQuery.java:148-189).  gf_traj_group is that
 * group-by for a device-resident window (needs pts->objID; n < 2^32):
 *   keys[ntraj]        the distinct objID keys in FIRST-OCCURRENCE order: trajectory t is the objID
 *                      whose first point has the t-th smallest index (Flink's keyBy emission order
 *                      is unspecified; this one never depends on scheduling);
 *   seg_off[ntraj + 1] segment offsets into perm;
 *   perm[n]            window indices, ascending inside each segment (arrival order).
 * Any int64 is a legal key (numeric, dictionary, GF_OBJID_NULL: a null objID is a group like any
 * other).  The result is identical from run to run.  Sync.  *out == NULL: a new groups object;
 * otherwise that object (of the same context) is regrouped and its device workspace reused. */
typedef struct gf_traj_groups gf_traj_groups;
int  gf_traj_group(gf_ctx* ctx, const gf_points* pts, gf_traj_groups** out);
void gf_traj_groups_destroy(gf_traj_groups* g);
int  gf_traj_groups_info(const gf_traj_groups* g, int64_t* ntraj, int64_t* n);
/* Sync: host copies of keys[ntraj], seg_off[ntraj + 1], perm[n]; any may be NULL. */
int  gf_traj_groups_read(gf_traj_groups* g, int64_t* keys, int64_t* seg_off, uint32_t* perm);
/* Testing / tuning: trajectories of at least `len` points take tStats' block-per-trajectory path
 * (len >= 1; 0 = the default, 2048).  Results are identical for any value. */
int  gf_traj_groups_set_long_threshold(gf_traj_groups* g, int64_t len);
/* TStatsQuery.TStatsQueryWFunction.apply (TStatsQuery.java:154-188) per trajectory, over its points
 * in arrival order (pts: the grouped window; needs x, y, ts):
 *   last = 0; for p: if (last == 0) { last = p.ts; X, Y = p; S = 0.0; T = 0 }
 *                    else if (p.ts > last) { S += sqrt(dy*dy + dx*dx); T += p.ts - last; last = p.ts; X, Y = p }
 *   row = (key, S, T, S / (double)T)        (DistanceFunctions.java:60-63; fewer than two counted
 *                                            points: 0.0, 0, NaN)
 * S is the sequential left-to-right binary64 sum, bit for bit.  Timestamps must be >= 0 (epoch
 * milliseconds): points with ts == 0 never count and a point counts iff its ts exceeds every
 * earlier ts of its trajectory; negative timestamps are outside the contract.
 * id_set (host, nset keys; PointTStatsQuery.java:76-84 trajIDSet): non-empty = only trajectories
 * whose key is in it.  Rows in first-occurrence order into HOST arrays (any may be NULL): *count =
 * all rows, at most cap written (as gf_bitmap_to_indices).  Sync. */
int  gf_tstats_run(gf_traj_groups* g, const gf_points* pts, const int64_t* id_set, int64_t nset,
                   int64_t* keys, double* spatial, int64_t* temporal, double* speed, int64_t cap, int64_t* count);
/* Sub-trajectories: every trajectory with at least one point flagged in `bitmap` (device
 * uint64[(n+63)/64], e.g. gf_range_run's), in full, as CSR in HOST arrays -- the assembly half of the
 * window-based tRange / tKnn / tJoin (PointPolygonTRangeQuery.java:158-176, PointPointTKNNQuery.java:
 * 241-270; single-point trajectories are emitted too, the caller applies the reference's size rules).
 * Trajectories in first-occurrence order: keys[m], off[m + 1]; trajectory j owns points
 * [off[j], off[j+1]) of x, y, ts, idx (idx = window index), in arrival order.  *ntraj_out = m and
 * *npts_out = all their points; at most cap_traj trajectories (keys, and off[0 .. min(m, cap_traj)])
 * and cap_pts points are written.  Any output array may be NULL.  Sync. */
int  gf_traj_select(gf_traj_groups* g, const gf_points* pts, const uint64_t* bitmap, int64_t* keys, int64_t* off,
                    int64_t cap_traj, double* x, double* y, int64_t* ts, uint32_t* idx, int64_t cap_pts,
                    int64_t* ntraj_out, int64_t* npts_out);

/* ---- tAggregate: the windowed heatmap ------------------------------------------------------
 * PointTAggregateQuery.java (QueryType.WindowBased, windowType "TIME") -> TAggregateQuery.java:498-613
 * TimeWindowProcessFunction.process, for one device-resident window.  The reference keys the window
 * by every point's cell-ID String and, per cell, walks the points in arrival order:
 *   first point of an objID:  min = max = ts, length 0
 *   repeat point:             min / max updated; length = max - min; sum follows the lengths;
 *                             if (length > maxLen) maxLen, maxKey = length, objID   (strict)
 *                             if (length < minLen) minLen, minKey = length, objID   (strict)
 * The cell of a point is K1's (cx, cy) (HelperClass.assignGridCellID, Java (int) saturation, NaN -> 0).
 * The reference's only filter is gridID != null, which every Point built with a grid passes: cells
 * outside the grid are cells like any other.  The key here is the int32 pair (cx, cy); it differs
 * from the "%05d%05d" String key only where an index needs more than five characters (Strings of
 * different pairs can then coincide).  Per cell c, with D_c its distinct objID keys (any int64 is a
 * legal key, as for gf_traj_group) and t_1 .. t_m the timestamps of objID o's points in c:
 *   L_o = max t - min t;   e_o = |t_2 - t_1|, s_o = the window index of o's second point   (m >= 2)
 *   f_o = the largest of s_o, the first index with ts == max t, the first index with ts == min t
 *   count  = |D_c|                     multi = the number of o with m >= 2
 *   sum    = the sum of L_o
 *   minLen = min e_o over m >= 2,      minKey = the o with e_o == minLen and the smallest s_o
 *   maxLen = max L_o over m >= 2,      maxKey = the o with L_o == maxLen and the smallest f_o
 * (the running length of an objID never decreases, so the strict `<` is decided at second points --
 * MIN is over e_o, not L_o, a quirk kept -- and the strict `>` by whoever reaches the final maximum
 * first).  With multi == 0: minLen = INT64_MAX, maxLen = INT64_MIN (the reference's initial values),
 * minKey = maxKey = 0.  Cells in the order of their first point in the window; inside a cell's ALL
 * rows, objIDs in the order of their first point in that cell (Flink's order is unspecified; this one
 * never depends on scheduling).  Timestamps >= 0 with sums inside int64; n < 2^32.  Results are
 * identical from run to run.
 * Not covered: the RealTime map function (TAggregateQuery.java:53-377, it reads the wall clock) and
 * windowType "COUNT"; no JNI binding.
 *
 * gf_tagg_group (needs x, y, objID): the (cell, objID) grouping.  *out == NULL: a new object;
 * otherwise that object (of the same context) is regrouped and its device workspace reused.  Sync.
 * gf_tagg_run (pts: the grouped window; needs ts): the statistics.  Sync. */
typedef struct gf_tagg gf_tagg;
int  gf_tagg_group(gf_ctx* ctx, const gf_grid* grid, const gf_points* pts, gf_tagg** out);
int  gf_tagg_run(gf_tagg* t, const gf_points* pts);
void gf_tagg_destroy(gf_tagg* t);
int  gf_tagg_info(const gf_tagg* t, int64_t* cells, int64_t* groups, int64_t* n);
/* Testing / tuning: (cell, objID) groups of at least long_group points and cells of at least
 * big_cell objIDs take the block-per-item paths (>= 1; 0 = the defaults, 2048 and 1024).  Takes effect
 * at the next gf_tagg_run; results are identical for any values. */
int  gf_tagg_set_thresholds(gf_tagg* t, int64_t long_group, int64_t big_cell);
/* After gf_tagg_run, the per-cell table into HOST arrays (any may be NULL): *cells = all cells, at
 * most cap written.  Sync. */
int  gf_tagg_read_cells(gf_tagg* t, int32_t* cx, int32_t* cy, int64_t* count, int64_t* multi, int64_t* sum,
                        int64_t* minLen, int64_t* minKey, int64_t* maxLen, int64_t* maxKey, int64_t cap, int64_t* cells);
/* After gf_tagg_run, the ALL rows as CSR into HOST arrays (any may be NULL): cell j owns
 * keys / len [off[j], off[j + 1]) = its {objID: L_o} map in first-point order.  *cells, *groups = the
 * full sizes; off[0 .. min(cells, cap_cells)] and at most cap_groups keys / len are written.  Sync. */
int  gf_tagg_read_all(gf_tagg* t, int64_t* off, int64_t* keys, int64_t* len, int64_t cap_cells, int64_t cap_groups,
                      int64_t* cells, int64_t* groups);
/* The emitted rows of one aggregate function from the per-cell table (pure host, no GPU): function
 * is compared as equalsIgnoreCase.  *kind = 0 ALL (and any unknown name), 1 SUM, 2 AVG, 3 MIN, 4 MAX.
 *   ALL  emit = 1, value = sum, key = 0 (the payload is the cell's gf_tagg_read_all map)
 *   SUM  emit = sum > 0,   value = sum                                            key = 0 (the "" key)
 *   AVG  emit = sum > 0,   value = Math.round((double)sum / (double)count)        key = 0
 *   MIN  emit = multi > 0, value = minLen, key = minKey
 *   MAX  emit = multi > 0, value = maxLen, key = maxKey
 * Rows not emitted have value = key = 0.  minLen .. maxKey are read only by MIN / MAX. */
int  gf_tagg_rows(const char* function, int64_t cells, const int64_t* count, const int64_t* multi, const int64_t* sum,
                  const int64_t* minLen, const int64_t* minKey, const int64_t* maxLen, const int64_t* maxKey,
                  uint8_t* emit, int64_t* value, int64_t* key, int32_t* kind);

/* ---- tKnn: the window-based trajectory kNN ---------------------------------------------------
 * tKnn/PointPointTKNNQuery.java windowBased (GF_TKNN_GRID, `run`) and windowBasedNaive (GF_TKNN_NAIVE,
 * `runNaive`) with TKNNQuery.java:50-101 kNNEvaluationWindowed, for one device-resident window of
 * n < 2^32 points already grouped by objID (gf_traj_group): the k trajectories nearest to the query
 * point (qx, qy).  Flink's emission orders are unspecified and the reference depends on them in three
 * places; this contract fixes each by first-occurrence order, never by scheduling.
 *  1. Cells.  A point's cell is K1's (cx, cy) (HelperClass.assignGridCellID, Java (int) saturation,
 *     NaN -> 0).  The cell set N:
 *       GRID, r != 0:  L = getCandidateNeighboringLayers(r); L <= 0 -> GF_ERR_LAYERS (as the join);
 *                      N = the cells with |cx - qcx| <= L, |cy - qcy| <= L and validKey
 *                      (UniformGrid.java:261-293), tested arithmetically per point
 *       GRID, r == 0:  N = every valid cell (girdCellsSet)
 *       NAIVE:         N = every cell a point falls in, cells outside the grid included; the key is
 *                      the int32 pair as for tAggregate, with its caveat about the String key
 *     Quirk kept: the window mode never compares a distance with r.
 *  2. Distance.  d_i = sqrt((qy - y_i) * (qy - y_i) + (qx - x_i) * (qx - x_i)), the sum in that order
 *     (DistanceFunctions.java:60-63), binary64 without FMA.  GF_METRIC_* does not apply: tKnn never
 *     goes through JTS.  A NaN distance is reported as Double.doubleToLongBits' NaN, 0x7ff8000000000000.
 *  3. Per (cell c in N, objID o), over o's points in c in window order (TKNNQuery.java:72-83: the first
 *     sets the value, a later one replaces it iff new < cur):  d(c, o) = NaN iff the first such point's
 *     distance is NaN, else the minimum of the non-NaN distances.
 *  4. Per cell the list L_c: its k smallest pairs by (d under Double.compareTo -- NaN last --, then
 *     the trajectory's rank t).  t = the trajectory's first-occurrence rank in the whole window
 *     (gf_traj_group's order); Java's tie order is HashMap iteration order.  The rank, not the key, on
 *     purpose: it does not depend on dictionary ids.
 *  5. Per trajectory t in at least one list: cells_t = the number of lists holding it, D_t = the least
 *     d(c, t) over THOSE lists under compareTo (NAIVE takes this minimum, :586-588; GRID takes the
 *     first record to arrive, :259-262, of which the least is the one legal outcome independent of
 *     arrival).  Not o's minimum over N: the truncation of step 4 happens first, and is observable.
 *  6. Size rule.  t is dropped unless it has >= 2 points in the WHOLE window (points outside N and
 *     outside the grid count: the join is against the unfiltered stream; the reference's
 *     coordinateList.size() > 1 with size = cells_t x len_t).
 *  7. Result: the k smallest survivors by (D_t under compareTo, t).  Per row: key, D_t, cells_t and the
 *     whole trajectory (x, y, ts, idx = window index, in arrival order) as CSR in result order.  The
 *     reference's LineString repeats the trajectory's points cells_t times (a join artefact); each point
 *     is emitted once here and cells_t reported.  Any int64 is a legal key.  Results are identical
 *     from run to run.
 *  8. k < 1, a NaN query coordinate, a NaN or negative r, an unknown mode, a null groups object / grid
 *     / pts / x / y / objID / ts, or pts that is not the grouped window: GF_ERR_ARG before any device
 *     call.  An empty N or an empty window: no rows, GF_OK.
 * Not covered: the RealTime paths, CountBased, sliding panes, sharding across GPUs, JNI bindings, the
 * non-point tKnn pairs.
 *
 * gf_tknn_run: *out == NULL: a new object; otherwise that object (of the groups' context) is reused with
 * its device workspace.  Sync.  gf_tknn_info: rows, their points, and what the window reached:
 * in_cells = points in N, pairs = distinct (cell, objID) pairs, records = the sum of |L_c|. */
#define GF_TKNN_GRID  0
#define GF_TKNN_NAIVE 1
typedef struct gf_tknn gf_tknn;
int  gf_tknn_run(gf_traj_groups* g, const gf_grid* grid, const gf_points* pts, double qx, double qy, double r,
                 int32_t k, int mode, gf_tknn** out);
void gf_tknn_destroy(gf_tknn* t);
int  gf_tknn_info(const gf_tknn* t, int64_t* rows, int64_t* npts, int64_t* in_cells, int64_t* pairs, int64_t* records);
/* The rows into HOST arrays (any may be NULL): at most cap_rows keys / dist / cells and
 * off[0 .. min(rows, cap_rows)], at most cap_pts points; the full counts are gf_tknn_info's.  Sync. */
int  gf_tknn_read(gf_tknn* t, int64_t* keys, double* dist, int32_t* cells, int64_t* off, int64_t cap_rows, double* x,
                  double* y, int64_t* ts, uint32_t* idx, int64_t cap_pts);
/* Testing / tuning: cells of at least big_cell pairs are ranked by one sort of all pairs, smaller ones
 * by counting inside the cell (>= 1; 0 = the default, 512).  Takes effect at the next gf_tknn_run;
 * results are identical for any value.  (The pair minima are order-free atomics for every pair, however
 * many points it holds: there is no long-pair path and so no threshold for one.) */
int  gf_tknn_set_thresholds(gf_tknn* t, int64_t big_cell);

/* ---- tJoin: the window-based trajectory join ---------------------------------------------------
 * tJoin/PointPointTJoinQuery.java windowBased (GF_TJOIN_PAIR, `run`) and commonSingle (GF_TJOIN_SINGLE,
 * `runSingle`, :341-435) with TJoinQuery.java, for one device-resident ordinary window O and one query
 * window Q, each already grouped by objID (gf_traj_group), n_o, n_q < 2^32, timestamps >= 0 (as for
 * tStats), one grid for both sides: the pairs of trajectories with a point of one within r of a point of
 * the other, each pair once, each trajectory whole.
 *  1. Matching point pairs: exactly the pair set of
 *       gf_join_pp(ctx, grid, grid, O, Q, r, approximate = 0, GF_METRIC_SQRT, ...).
 *     q is replicated to getNeighboringCells(r, q) (UniformGrid.java:261-293): the valid cells within
 *     L = getCandidateNeighboringLayers(r) layers of q's cell (q itself may lie outside the grid); r == 0:
 *     every valid cell.  L <= 0 -> GF_ERR_LAYERS.  p joins on its own cell, which must be a valid cell.  A
 *     pair survives iff getPointPointEuclideanDistance(p, q) <= r, binary64 without FMA: the sum of the
 *     two squares commutes, so the value is bit-identical to GF_METRIC_SQRT's.  NaN never matches.
 *  2. Rows: the distinct (t_o, t_q) with at least one matching pair (p of t_o, q of t_q), t = the
 *     trajectory's first-occurrence rank in its own window (gf_traj_group's order), ascending by
 *     (t_o, t_q).  Flink's emission order is unspecified; this is the fixed one.
 *  3. Row fields.  okey, qkey: the objID keys (any int64 is a legal key).
 *     q_latest: the window index of the matching q of t_q with the largest ts, among equal ts the smallest
 *       index -- the secondIDPointMap loop (PointPointTJoinQuery.java:263-281) replaces iff
 *       new.ts > old.ts, so the first arrival wins a tie; arrival is fixed as the query window's order.
 *     p_first: the smallest ordinary window index of t_o matching any point of t_q.  The reference's
 *       firstPoint of an ordinary objID (the ordinary point of the first pair to arrive for it; arrival
 *       fixed as the ordinary window's order) is the minimum of p_first over that objID's rows.
 *  4. Size rule.  emit = (t_o has >= 2 points in the WHOLE of O) and (t_q has >= 2 in the whole of Q)
 *     (GenerateWindowedTrajectory, TJoinQuery.java:184: the two joins against the trajectory streams drop
 *     the rest; points outside the grid count).  Rows with emit = 0 stay in the row table -- they are
 *     runSingle's Point-pair output -- and own no trajectory in the CSR.
 *  5. Trajectories.  Per side the distinct trajectories of the emitted rows, ascending rank, each whole
 *     and once, as CSR: keys[m], off[m + 1], x, y, ts, idx (window index) in arrival order.  An emitted
 *     row carries oslot / qslot, its positions in those two lists (emit = 0: -1).  The reference emits a
 *     Tuple2<LineString, LineString> per row; this is that without copying a trajectory per partner.
 *  6. GF_TJOIN_SINGLE: one window against itself; go == gq (the same object) and rows of equal objID are
 *     excluded.  Deviation: the reference writes `p.objID != q.objID` on Strings, a reference comparison
 *     whose outcome depends on JVM object identity after serialisation; a C ABI cannot express that, and
 *     the evident intent ("no need to join a trajectory with itself") is kept.
 *  7. A NaN r, an unknown mode, a null object / grid / pts / x / y / objID / ts (either side), groups of
 *     different contexts, pts that are not the grouped windows, SINGLE with two different groups objects:
 *     GF_ERR_ARG before any device call.  An empty window on either side: no rows, GF_OK.  Results are
 *     identical from run to run.
 * Not covered: the RealTime paths and their triggers, realTimeJoinNaive, sliding panes, sharding across
 * GPUs, JNI bindings.
 *
 * gf_tjoin_run: *out == NULL: a new object; otherwise that object (of the groups' context) is reused, its
 * device workspace grow-only.  The rows are collected in a device hash table whose size is not known
 * beforehand: it starts from the object's previous window (or a default), and when a probe finds it more
 * than half full the library doubles it and probes again -- the caller sees no capacity error, only
 * probe_passes; GF_ERR_NOMEM when the table would outgrow what min(n_o x n_q, free memory) allows.  Sync.
 * gf_tjoin_info: rows, emitted rows, the CSRs' trajectories and points per side, probe runs of the last
 * call. */
#define GF_TJOIN_PAIR 0
#define GF_TJOIN_SINGLE 1
typedef struct gf_tjoin gf_tjoin;
int  gf_tjoin_run(gf_traj_groups* go, const gf_points* opts, gf_traj_groups* gq, const gf_points* qpts,
                  const gf_grid* grid, double r, int mode, gf_tjoin** out);
void gf_tjoin_destroy(gf_tjoin* t);
int  gf_tjoin_info(const gf_tjoin* t, int64_t* rows, int64_t* emitted, int64_t* otraj, int64_t* opoints,
                   int64_t* qtraj, int64_t* qpoints, int64_t* probe_passes);
/* The row table into HOST arrays (any may be NULL): at most cap rows; the full count is gf_tjoin_info's.  Sync. */
int  gf_tjoin_read_rows(gf_tjoin* t, int64_t* okey, int64_t* qkey, uint32_t* p_first, uint32_t* q_latest,
                        uint8_t* emit, int32_t* oslot, int32_t* qslot, int64_t cap);
/* One side's CSR (0 ordinary, 1 query) into HOST arrays (any may be NULL): at most cap_traj keys and
 * off[0 .. min(m, cap_traj)], at most cap_pts points.  Sync. */
int  gf_tjoin_read_trajs(gf_tjoin* t, int side, int64_t* keys, int64_t* off, int64_t cap_traj,
                         double* x, double* y, int64_t* ts, uint32_t* idx, int64_t cap_pts);
/* Testing: the table's size at the next gf_tjoin_run (a power of two >= 16; 0 = the default).  Results are
 * identical for any value. */
int  gf_tjoin_set_table_slots(gf_tjoin* t, int64_t slots);

/* ---- tRange / tFilter: trajectories that enter a polygon set, trajectories of an id set -------
 * tRange/PointPolygonTRangeQuery.java and tFilter/PointTFilterQuery.java for one device-resident
 * window.  The contract (derived from the reference and JTS 1.16.1, nothing was run on a JVM):
 *  1. contains.  A point p is contained by a polygon iff `poly.polygon.contains(p.point.getEnvelope())`
 *     (PointPolygonTRangeQuery.java:81,130), JTS Geometry.contains: false unless the polygon's (shell)
 *     envelope holds p -- so a NaN or infinite coordinate is never contained -- then RectangleContains
 *     for a rectangle (the strict interior of the box) or relate(p).isContains(), i.e. PointLocator
 *     locates p INTERIOR: INTERIOR of the shell and neither INTERIOR nor BOUNDARY of any hole.  Both
 *     branches agree: contained iff located INTERIOR.  A point on a shell or hole edge is NOT contained
 *     (a range plan computes distance <= r: at a tiny positive r the closed polygon, which keeps such a
 *     point; at r = 0 it has no candidate cells at all and returns nothing).
 *     The ring walk is RayCrossingCounter with the exact orientation sign (RobustDeterminant).
 *  2. The cell filter is a pure prune.  The reference keeps a point only if its gridID is among the
 *     polygons' bbox cells (HelperClass.java:123-143).  A contained point lies strictly inside the bbox
 *     and the cell index is monotone in the coordinate (Java's saturation included), so its cell is in
 *     the set: filter + contains == contains, for points and polygons outside the grid too.  The plan's
 *     cell table only skips work.
 *  3. gf_trange_points (RealTime, :53-87): bit i of bitmap (device uint64[(n+63)/64], every word
 *     written) = point i is contained by some polygon of the set; *count (device int64, nullable) =
 *     the number of set bits.  Enqueued on the context stream like gf_range_run; needs x and y only.
 *  4. gf_trange_run (WindowBased, :89-176): the trajectories (objIDs of the window grouped by
 *     gf_traj_group) with at least one contained point, each whole, in first-occurrence order, points in
 *     arrival order -- outputs exactly as gf_traj_select (single-point trajectories included; the caller
 *     applies the reference's size rule).  Sync.  A trajectory already known to be hit skips its
 *     remaining points' tests; which points were skipped depends on scheduling, the result never does.
 *  5. gf_tfilter_run (PointTFilterQuery.java windowBased): the trajectories whose objID key is in id_set
 *     (host, nset keys, duplicates allowed), each whole; nset == 0 = every trajectory (:92-95).  Outputs
 *     as gf_traj_select.  Sync.
 *  6. Errors: null plan / groups / pts / required pointer, negative capacities, npoly < 0, an invalid
 *     grid or ring, pts that is not the grouped window, a plan and groups of different contexts:
 *     GF_ERR_ARG before any device call.  An empty polygon set, an empty window and ntraj == 0 return
 *     zero rows (bitmap: all zero).
 * Not covered: Flink's triggers and sliding assignment, the RealTime tFilter's watermarking, sharding
 * across GPUs, JNI bindings.
 * The plan (once per continuous query): per grid cell a class -- none (no bbox covers it), test (the CSR
 * list of the polygons whose bbox cells cover it), inside (the cell's whole coordinate extent lies
 * strictly inside a rectangle polygon: every non-NaN point of it is contained untested) -- plus the
 * polygons whose bbox cells leave the grid, for the points whose cell is outside it.
 * gf_trange_plan_stats: cells per class, the list entries, and the polygons whose largest ring has at
 * least `wide_ring` vertices: those are tested by one wave per (point, polygon) instead of one lane
 * (gf_trange_plan_set_thresholds: wide_ring >= 1; 0 = the default, 384; results are identical for any
 * value).  The wave path's worklist lives in the plan and only grows: n times the most wide polygons any
 * one cell's list holds, 8 B each.  A window larger than every earlier one makes gf_trange_points and
 * gf_trange_run synchronise the stream and allocate before they enqueue; a window whose bound exceeds
 * 1 GiB is tested by lanes only (identical results).  gf_trange_info: of the last gf_trange_run, the points
 * whose cell class is not none and those in inside cells (both independent of scheduling); the wide_ring
 * in force; and wave_path = 1 iff the last gf_trange_points / gf_trange_run tested its wide polygons by
 * waves (0: the set has none, or the worklist bound was too large).  Any output may be NULL. */
typedef struct gf_trange_plan gf_trange_plan;
int  gf_trange_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_polygons* polys, gf_trange_plan** out);
void gf_trange_plan_destroy(gf_trange_plan* p);
int  gf_trange_plan_stats(const gf_trange_plan* p, int64_t* none_cells, int64_t* test_cells, int64_t* inside_cells,
                          int64_t* list_entries, int64_t* wide_polygons);
int  gf_trange_plan_set_thresholds(gf_trange_plan* p, int32_t wide_ring);
int  gf_trange_points(gf_trange_plan* p, const gf_points* pts, uint64_t* bitmap, int64_t* count);
int  gf_trange_run(gf_trange_plan* p, gf_traj_groups* g, const gf_points* pts, int64_t* keys, int64_t* off,
                   int64_t cap_traj, double* x, double* y, int64_t* ts, uint32_t* idx, int64_t cap_pts,
                   int64_t* ntraj_out, int64_t* npts_out);
int  gf_trange_info(const gf_trange_plan* p, int64_t* cell_points, int64_t* inside_points, int64_t* wide_ring,
                    int64_t* wave_path);
int  gf_tfilter_run(gf_traj_groups* g, const gf_points* pts, const int64_t* id_set, int64_t nset, int64_t* keys,
                    int64_t* off, int64_t cap_traj, double* x, double* y, int64_t* ts, uint32_t* idx, int64_t cap_pts,
                    int64_t* ntraj_out, int64_t* npts_out);

/* ---- polygon and linestring windows: range and kNN against query points ----------------------
 * range/PolygonPointRangeQuery.java:116-196, range/LineStringPointRangeQuery.java:118-191,
 * knn/PolygonPointKNNQuery.java:136-209, knn/LineStringPointKNNQuery.java:136-206 (WindowBased) with
 * KNNQuery.kNNWinAllEvaluationPolygonStream: the WINDOW holds geometries, the query is a point set.
 * The contract (derived from the reference and JTS 1.16.1, nothing was run on a JVM):
 *  1. Window objects.  A window holds nobj objects of one kind (gf_geoms, device CSR).  A polygon is
 *     its rings, ring 0 the shell, every ring closed with >= 4 vertices (as gf_polygons); a linestring
 *     is an open chain of >= 2 vertices (as gf_linestrings).  boundingBox = the vertex envelope, for a
 *     polygon its shell's (JTS).  gridIDsSet = HelperClass.assignGridCellID(bbox) (HelperClass.java:
 *     123-143; holes are taken to lie inside the shell's envelope, as in a valid JTS polygon -- the
 *     exact pass skips an object whose SHELL envelope is provably farther than r): the rectangle of cells [cx1..cx2] x [cy1..cy2] of the envelope's corners, each index
 *     K1's floor with Java (int) saturation, NOT clamped to the grid.  A cell outside the grid belongs
 *     to no neighbour set (UniformGrid.validKey).
 *  2. Query side.  N = the union over the query points of getNeighboringCells(r, point): the valid
 *     cells within L = getCandidateNeighboringLayers(r) layers of the point's cell (the point may lie
 *     outside the grid: its cell index is used as it is, as the point plans do); r == 0: N = every
 *     valid cell; r != 0 and L <= 0: GF_ERR_LAYERS (the reference's System.exit(1)).  G = the union of
 *     getGuaranteedNeighboringCells(r, point.gridID): layers -1 -> nothing, 0 -> the point's cell,
 *     g > 0 -> the valid cells within g layers.
 *  3. Range.  An object passes the filter iff some cell of its rectangle is in N.  A filtered object
 *     is emitted, once, iff (a) every cell of its rectangle is in G, or (b) not (a) and some query
 *     point has d <= r.  The Java loop over the HashSet counts G cells and leaves at the first cell
 *     outside G with the distance test, emitting at the last cell only when all were in G: the result
 *     does not depend on the set's iteration order.  A rectangle that leaves the grid is never all-G.
 *     Exact: d = DistanceFunctions.getDistance(point, polygon) -- the JTS point-polygon distance, 0
 *     inside -- or getDistance(point, lineString), the open-chain minimum with no containment; either
 *     metric.  Approximate: d = getPointPolygonBBoxMinEuclideanDistance /
 *     getPointLineStringBBoxMinEuclideanDistance on the object's own envelope.
 *  4. kNN.  One query point.  Candidates: the objects with a rectangle cell in N (G is not used) and
 *     d <= r, d as in 3.  The record is the library's kNN record contract, not the reference's
 *     arrival-order ties: entries sorted by (d, objID key, idx), one entry per objID key holding its
 *     smallest d (among equal d the smallest idx), at most k entries, idx = the object's index in the
 *     window.  The reference keys polygons by "" (one heap, then the dedupe of KNNQuery) and
 *     linestrings by the matched cell (per-cell heaps, then the same merge): both collapse to this.
 *     A plain gf_knn_header record, status always 0 (no hint, no fallback): gf_knn_merge_dev(_batch)
 *     and record decoding take it unchanged.  k <= 512: the one-block select; larger k: the sorted path.
 *  5. Errors, before any device call: a null handle or required pointer, nobj < 0, nq <= 0, k < 1, a
 *     kNN query with nq != 1, a window prepared on another grid or context than the query's, a kind
 *     other than the two, a bad metric, a grid of more than 46340 partitions (the summed-area tables
 *     are int32): GF_ERR_ARG.  An empty window: an all-zero bitmap / a record with n = 0.
 *  6. An object with a ring of fewer than 4 vertices, an unclosed ring, no ring at all, or a chain of
 *     fewer than 2 vertices is never selected; gf_geom_prepare counts such objects (`invalid`).  The
 *     reference leaves a null JTS object and throws later.  Non-finite vertex coordinates are outside
 *     this contract.  The offset arrays are trusted to be monotone and in bounds, as gf_points.n is.
 * Not covered: RealTime mode, Flink's triggers and sliding assignment, sharding across GPUs, JNI.
 * (Polygon and linestring QUERIES against these windows: the next block.)
 *
 * gf_geoms: polygons -- object i owns rings [ring_off[i], ring_off[i+1]); ring j owns vertices
 * [vert_off[j], vert_off[j+1]).  Linestrings -- ring_off == NULL, object i owns vertices
 * [vert_off[i], vert_off[i+1]).  Every pointer is a DEVICE pointer.  vx / vy may be NULL only when the
 * window holds no vertex at all (every object is then invalid).
 * gf_geom_prepare (async; once per window, its index reusable by many queries of the same context and
 * grid): per ring its envelope, per object its envelope, cell rectangle, validity and vertex count.
 * *out == NULL: a new index; otherwise that index (of the same context) is prepared again for the new
 * window -- its threshold kept, its device arrays reused and grow-only -- which is the per-window path of
 * a continuous query.  Only launches are enqueued, with no host read (geoms->nrings carries the ring
 * count); a new index, or a window with more objects or rings than the index has held, first synchronises
 * the stream and allocates, as gf_trange_points does for its worklist.  The window's arrays are borrowed:
 * they must stay valid and unchanged while the index is in use.
 * One stream: an index holds the worklists of the run in flight and a query its counters and kNN
 * candidates, so every call on an index or a query must be enqueued on the context stream (runs of
 * several queries on one index are then ordered); running them from the streams gf_ctx_fork orders
 * would race.
 * Objects of at least wide_vertices vertices (gf_geom_index_set_thresholds; 0 = the default, 384; >= 1)
 * are tested by one wave instead of one lane, and rings of at least as many have their envelope taken
 * by one wave; results are identical for any value.  gf_geom_index_info (sync): objects, vertices,
 * invalid objects, objects at or above the threshold.  gf_geom_index_read (sync, tests): env = x1, y1,
 * x2, y2 per object; cells = cx1, cy1, cx2, cy2 per object.
 * gf_geom_query_create (once per continuous query): the per-cell N / G tables of the point set and
 * their summed-area tables, so "some cell in N" and "every cell in G" are two rectangle sums for any nq.
 * gf_geom_range_run (async): bitmap = device uint64[(nobj+63)/64], gf_range_run's layout, every word
 * written (gf_bitmap_to_indices(_async) take it); counts (nullable) = device int64[2]: objects
 * emitted, and those emitted through rule 3(a).
 * gf_geom_knn_enqueue (async): one record of gf_knn_result_bytes(k) into device memory `result`;
 * needs geoms->objID.
 * gf_geom_info (sync, of the query's last run): objects that passed the filter, those all-G, those
 * whose distance was evaluated (the exact passes' worklists), and those of them tested by a wave. */
#define GF_GEOM_POLYGON    1
#define GF_GEOM_LINESTRING 2
typedef struct {
  int32_t kind;
  int32_t nrings;        /* polygons: the rings of the window, ring_off[nobj] (trusted, as the offsets); linestrings: unused */
  int64_t nobj;
  const int32_t* ring_off;
  const int32_t* vert_off;
  const double* vx;
  const double* vy;
  const int64_t* objID;  /* objID keys; kNN only */
  const int64_t* ts;     /* never read by window evaluation */
} gf_geoms;
typedef struct gf_geom_index gf_geom_index;
int  gf_geom_prepare(gf_ctx* ctx, const gf_grid* g, const gf_geoms* geoms, gf_geom_index** out);
void gf_geom_index_destroy(gf_geom_index* ix);
int  gf_geom_index_info(gf_geom_index* ix, int64_t* nobj, int64_t* nvert, int64_t* invalid, int64_t* wide);
int  gf_geom_index_read(gf_geom_index* ix, double* env, int32_t* cells);
int  gf_geom_index_set_thresholds(gf_geom_index* ix, int32_t wide_vertices);
typedef struct gf_geom_query gf_geom_query;
int  gf_geom_query_create(gf_ctx* ctx, const gf_grid* g, const double* qx, const double* qy, int32_t nq, double r,
                          int approximate, int metric, gf_geom_query** out);
void gf_geom_query_destroy(gf_geom_query* q);
int  gf_geom_range_run(gf_geom_query* q, gf_geom_index* ix, uint64_t* bitmap, int64_t* counts);
int  gf_geom_knn_enqueue(gf_geom_query* q, gf_geom_index* ix, int32_t k, void* result);
int  gf_geom_info(const gf_geom_query* q, int64_t* filtered, int64_t* all_guaranteed, int64_t* tested,
                  int64_t* wave_path);

/* ---- geometry windows against polygon and linestring queries: range and kNN --------------------
 * range/PolygonPolygonRangeQuery.java:110-193, PolygonLineStringRangeQuery.java:111-197,
 * LineStringPolygonRangeQuery.java, LineStringLineStringRangeQuery.java:148-193 and
 * knn/PolygonPolygonKNNQuery.java:139-213, PolygonLineStringKNNQuery.java, LineStringPolygonKNNQuery.java,
 * LineStringLineStringKNNQuery.java (WindowBased): the WINDOW holds geometries (block above, rules 1 and
 * 6), the query is a set of polygons or of linestrings.  Four pairs of kinds, one gf_geom_query: it runs
 * through gf_geom_range_run, gf_geom_knn_enqueue, gf_geom_info and gf_geom_query_destroy against an index
 * of either window kind.  The contract (derived from the reference and JTS 1.16.1, nothing was run on a JVM):
 *  1. Query geometries.  nq >= 1 geometries of ONE kind (kNN: exactly one), host CSR (gf_polygons /
 *     gf_linestrings).  Each carries boundingBox and gridIDsSet exactly as a window object does: the
 *     shell's / the chain's vertex envelope, and the unclamped cell rectangle R_q =
 *     HelperClass.assignGridCellID(bbox).
 *  2. Query side.  g = getGuaranteedNeighboringLayers(r), c = getCandidateNeighboringLayers(r).  The
 *     operators' loop (PolygonPolygonRangeQuery.java:118-128; UniformGrid.java:193-222, 399-426) gives
 *       G = the union over the queries and over every cell of R_q of getGuaranteedNeighboringCells(r, cell):
 *           g < 0 nothing; g == 0 the cell itself with NO validKey (UniformGrid.java:171-174), so the cells
 *           of R_q outside the grid are members; g > 0 the valid cells within g layers;
 *       N = G u C, C = the valid cells within c layers of a cell of R_q, only when c > 0.
 *     These are NOT the point-query rules of the block above: (a) getNeighboringCells is never called, so
 *     there is no GF_ERR_LAYERS -- c <= 0 is an empty C; (b) r == 0 (c = 0, g = -1) gives N = {} and
 *     selects nothing, it does not select the whole grid.  A negative or NaN r selects nothing either.
 *     Cells are (cx, cy) pairs in or out of the grid; indices saturate like Java (int).
 *     Deviation: g == 0 with nq > 1 and some R_q leaving the grid -- G outside the grid is then a union of
 *     rectangles, whose cover test is not implemented -- is refused by create with GF_ERR_ARG.  With
 *     nq == 1 the out-of-grid members of G and N are the rectangle R_q itself and are handled exactly: an
 *     object has a cell in N iff the tables say so or its rectangle meets R_q, and all its cells in G iff
 *     the tables say so or its rectangle lies within R_q.
 *  3. Range.  Rule 3 of the block above, word for word, with these N and G: the filter (some rectangle
 *     cell in N), then emitted once iff every rectangle cell is in G, or else the first query of the set,
 *     in order, with d <= r.  Exact: d = DistanceFunctions.getDistance(query, object), rule 5, either
 *     metric.  Approximate: d = getBBoxBBoxMinEuclideanDistance(query.boundingBox, object.boundingBox)
 *     (DistanceFunctions.java:298-361; the query's box FIRST in all eight operators -- the kNN operators'
 *     getPolygonPolygonBBox... / getPolygonLineStringBBox... wrappers pass (query, object) on): with the
 *     query box (x1, y1, x2, y2) and the object box (p1, q1, p2, q2),
 *       p2 <= x1: q2 <= y1 -> |(x1, y1) (p2, q2)|; q1 >= y2 -> |(x1, y2) (p2, q1)|; else border((p2, q1); x = x1)
 *       p1 >= x2: q2 <= y1 -> |(x2, y1) (p1, q2)|; q1 >= y2 -> |(x2, y2) (p1, q1)|; else border((p1, q1); x = x2)
 *       else:     q2 <= y1 -> border((p1, q2); y = y1);  q1 >= y2 -> border((p1, q1); y = y2);  else 0,
 *     border = getPointLineStringNearestBBoxBorderMinEuclideanDistance (its x1 == x2 test first), distances
 *     sqrt(dy*dy + dx*dx) whatever `metric` says.
 *  4. kNN.  One query.  Candidates: the objects with a rectangle cell in N (G unused) and d <= r.  The
 *     record: rule 4 of the block above, unchanged.
 *  5. The exact distance: JTS Geometry.distance -> DistanceOp(query, object), terminate distance 0.
 *     (a) Containment, both ways: for a query polygon, the object's FIRST coordinate (first shell vertex /
 *         first chain vertex; ConnectedElementLocationFilter) located by PointLocator -- not EXTERIOR
 *         (boundary counts as inside, inside a hole is exterior) -> d = 0; then the same with the query's
 *         first coordinate in an object polygon.  A linestring never contains anything, closed or not.
 *     (b) Otherwise the minimum, by `d < md`, over every (query ring or chain, object ring or chain) and
 *         every pair of their segments of Distance.segmentToSegment(A, B, C, D), AB the query's:
 *         A == B -> pointToSegment(A, C, D); C == D -> pointToSegment(D, A, B); the envelopes of AB and CD
 *         disjoint -> no intersection; else denom = (B.x-A.x)(D.y-C.y) - (B.y-A.y)(D.x-C.x), denom == 0 ->
 *         no intersection, else r = ((A.y-C.y)(D.x-C.x) - (A.x-C.x)(D.y-C.y)) / denom, s = ((A.y-C.y)(B.x-A.x)
 *         - (A.x-C.x)(B.y-A.y)) / denom, no intersection iff r < 0 || r > 1 || s < 0 || s > 1.  No
 *         intersection -> the minimum of pointToSegment(A, C, D), (B, C, D), (C, A, B), (D, A, B); otherwise
 *         0.0.  pointToSegment and the point-point distance under `metric` are those of the block above.
 *         JTS stops at md <= 0 and skips a pair of lines whose envelope distance exceeds the minimum so
 *         far; the contract is the plain minimum (the skip can change JTS's own result only
 *         through rounding, by a few ulp, in one branch).
 *     (c) Assumption: every hole of a polygon, query or object, lies inside its shell's envelope, as in a
 *         valid JTS polygon (rule 1 of the block above).  A query is not walked for an object whose
 *         boundingBox -- the SHELL's envelope -- is provably farther than r from the query's; a polygon with
 *         a hole outside its shell's envelope may therefore be reported farther than the plain minimum.
 *  6. Errors, before any device call: rule 5 of the block above, and a query set with nq < 1, a null
 *     array, offsets not starting at 0, a polygon without a ring, a ring of fewer than 4 vertices or
 *     unclosed, or a chain of fewer than 2 vertices: GF_ERR_ARG from create.  The refusal of rule 2.
 *     Invalid WINDOW objects: rule 6 of the block above.
 * Not covered: RealTime mode, sliding panes, sharding, JNI.  (The geometry-stream joins: the next block.)
 *
 * gf_geom_query_create_polygons / _linestrings (once per continuous query): the N / G tables of the
 * rectangles, the query CSR, per ring its envelope and the envelopes of its runs of 32 segments (as the
 * linestring plans cut theirs), per query its boundingBox and rectangle.
 * gf_geom_query_set_chain_mode (tests, tools): 0 = the run envelopes prune (default), 1 = no run envelope
 * is consulted; results are identical.  GF_ERR_ARG for a point query.
 * Objects of at least wide_vertices vertices are tested by one wave whose lanes stride the OBJECT's
 * segments; results are identical for any value.  gf_geom_info reads as for a point query. */
int  gf_geom_query_create_polygons(gf_ctx* ctx, const gf_grid* g, const gf_polygons* polys, double r, int approximate,
                                   int metric, gf_geom_query** out);
int  gf_geom_query_create_linestrings(gf_ctx* ctx, const gf_grid* g, const gf_linestrings* lines, double r,
                                      int approximate, int metric, gf_geom_query** out);
int  gf_geom_query_set_chain_mode(gf_geom_query* q, int mode);

/* ---- geometry-stream joins: polygon and linestring windows joined with a second stream -----------
 * join/PolygonPointJoinQuery.java, LineStringPointJoinQuery.java, PolygonPolygonJoinQuery.java,
 * PolygonLineStringJoinQuery.java, LineStringPolygonJoinQuery.java, LineStringLineStringJoinQuery.java with
 * JoinQuery.java:73-137, HelperClass.java:325-376 and UniformGrid.java:165-293, 368-445.  The contract
 * (derived from the reference and JTS 1.16.1, nothing was run on a JVM):
 *  1. Sides.  The ORDINARY side is a geometry window (gf_geoms) whose gf_geom_index was prepared on ugrid.
 *     The QUERY side is a point window (gf_points, with qgrid passed alongside) or a second geometry window
 *     whose own index was prepared on qgrid.  The two grids may differ, as in the point-point join: cell
 *     keys are compared as (cx, cy) index pairs, and "valid cell" means valid on qgrid.  Both indexes
 *     belong to one context.  Rules 1 and 6 of the geometry-window block hold for both sides: the cell
 *     rectangle R is unclamped, and an invalid object on either side is never paired.
 *  2. Replication.  Ordinary object o goes to every cell of R_o (ReplicatePolygonStreamUsingObjID /
 *     ReplicateLineStringStreamUsingObjID), valid or not.  With g the guaranteed and c the candidate layers
 *     of r on qgrid, query q goes to the cell set K(q):
 *       a point query: getNeighboringCells(r, q) -- r == 0: every valid cell; r != 0 and c <= 0 (a negative
 *         or NaN r): GF_ERR_LAYERS; otherwise the valid cells within c layers of the point's cell, which may
 *         itself lie outside the grid;
 *       a geometry query: G u C of getReplicated{Polygon,LineString}QueryStream -- the valid cells within c
 *         layers of some cell of R_q (only when c > 0), and, when g == 0, every cell of R_q with NO validKey,
 *         so its cells outside the grid are members.  (The g > 0 set lies inside the c set: g < c always.)
 *         r <= 0 or NaN gives K = {}: no pairs and no error -- rule 2(b) of the block above, not the point rule.
 *     The union of Chebyshev balls over a rectangle is a rectangle, so the in-grid part of K(q) is
 *       E_q = [x1 - c, x2 + c] x [y1 - c, y2 + c] n [0, n)^2,
 *     expanded in 64-bit arithmetic.  Deviation: Java's int sums wrap on saturated indices (a rectangle at
 *     Integer.MAX_VALUE grows into negative cells); here it grows past the index range and is clipped.
 *  3. Multiplicity.  Flink's equi-join emits a matching pair once per shared key:
 *       m(o, q) = |R_o n K(q)| = |R_o n E_q| + [geometry query and g == 0] (|R_o n R_q| - |R_o n R_q n grid|).
 *     A pair is a candidate iff m > 0.  m is reported per pair as min(m, 2^32 - 1) and computed without
 *     overflow (a side can be 2^32 cells long); *nrep sums the reported values.
 *  4. Test.  A candidate is emitted iff d <= r.
 *     Exact d, point query: getDistance(q, polygon), rule 3 of the geometry-window block, or
 *       getDistance(q, lineString), the open-chain minimum; either metric.
 *     Exact d, geometry query: rule 5 of the block above with the operator's own argument order -- the query
 *       is the FIRST geometry in PolygonPolygon, LineStringLineString and LineStringPolygon; in
 *       PolygonLineStringJoinQuery the ordinary polygon is first (getDistance(poly, q), lines 161-163).
 *       segmentToSegment(A, B, C, D) takes AB from the first geometry.
 *     Approximate d: getPointPolygonBBoxMinEuclideanDistance / getPointLineStringBBoxMinEuclideanDistance on
 *       the object's envelope for a point query; getBBoxBBoxMinEuclideanDistance(first.boundingBox,
 *       second.boundingBox) with the same first and second for a geometry query -- the function depends on
 *       the argument order for degenerate boxes.  Unlike the point-point join, approximate mode still tests
 *       d <= r.
 *  5. Result.  An unordered list of distinct (ordinary idx, query idx, m) triples.  RealTime mode calls
 *     windowBased with slide = size in all six operators: one window evaluation serves both.
 *  6. Errors, before any device call: a null handle or required pointer, indexes of another context than the
 *     joiner's, a bad metric, a negative cap, a null `pairs` with cap > 0, first_is_ordinary set for
 *     anything but a polygon ordinary side and a linestring query side: GF_ERR_ARG.  GF_ERR_LAYERS: rule 2.
 *     An empty window on either side: no pairs, GF_OK.
 * Not covered: run envelopes for the first geometry (a long first geometry is walked plainly behind the
 * box test), a wave form that strides the first geometry, balancing a lane that lands in a dense tile,
 * sliding panes, sharding, JNI.
 *
 * gf_geom_join_create / _destroy: the joiner owns the grow-only scratch of a run (the object and query lists,
 * the tile CSR, the candidate list) and is reused across windows; like an index it lives on the context
 * stream.
 * gf_geom_join_run / _run_points (sync, like gf_join_ppoly_run): pairs = device uint32[3 * cap], (o, q, m) per
 * pair, at most cap of them written; *npairs = the exact number of distinct pairs, *nrep = the sum of their
 * m; GF_ERR_CAPACITY iff *npairs > cap (pairs may be null with cap 0, to count).  first_is_ordinary: rule
 * 4's PolygonLineString order.  Tiles of T x T cells bin the short queries (E_q over at most long_tiles
 * tiles, no member of K outside the grid) into a CSR; one lane per short object walks the tiles of R_o and
 * takes a pair only at the tile holding the lower corner of R_o n E_q; long objects and long queries go
 * through a rectangle pass over pairs.  Exact mode then tests each candidate whose boxes are not provably
 * farther apart than r by one lane, or by one wave when the SECOND geometry (a point query: the object) has
 * at least its index's wide_vertices vertices.
 * gf_geom_join_info (of the last run): pairs with m > 0; exact mode: those dropped by the box test, those
 * whose distance was evaluated, and those of them by a wave (approximate mode decides in the probe: all
 * three are 0); objects and queries classed long.
 * gf_geom_join_set_tuning (tests, tools): tile_side (rounded up to a power of two; 0 = the smallest power of
 * two >= min(2c + 1, n); either is doubled until the grid has at most 1024 tiles a side), long_tiles (0 =
 * the default, 16), brute = 1: every pair through the rectangle pass.  Results never depend on it. */
typedef struct gf_geom_join gf_geom_join;
int  gf_geom_join_create(gf_ctx* ctx, gf_geom_join** out);
void gf_geom_join_destroy(gf_geom_join* j);
int  gf_geom_join_run(gf_geom_join* j, gf_geom_index* ix_ord, gf_geom_index* ix_qry, double r, int approximate, int metric,
                      int first_is_ordinary, uint32_t* pairs, int64_t cap, int64_t* npairs, int64_t* nrep);
int  gf_geom_join_run_points(gf_geom_join* j, gf_geom_index* ix_ord, const gf_grid* qgrid, const gf_points* q, double r,
                             int approximate, int metric, uint32_t* pairs, int64_t cap, int64_t* npairs, int64_t* nrep);
int  gf_geom_join_info(const gf_geom_join* j, int64_t* candidates, int64_t* box_dropped, int64_t* tested,
                       int64_t* wave_path, int64_t* long_objects, int64_t* long_queries);
int  gf_geom_join_set_tuning(gf_geom_join* j, int32_t tile_side, int64_t long_tiles, int brute);

/* ---- pinned host memory ---------------------------------------------------------------
 * Mapped, portable host memory: kernels write kNN records straight into it (pass it as the
 * `result` of gf_knn_enqueue), so no copy kernel runs per window. */
int  gf_pinned_alloc(size_t bytes, void** ptr);
void gf_pinned_free(void* ptr);

/* ---- host windows -------------------------------------------------------------------- */
typedef struct gf_window gf_window;
/* Library-owned device SoA window (reused across windows: create once per plan / operator).
 * gf_window_upload copies on the window's own stream, after the work already enqueued on the
 * context (which may still read the old contents) and without blocking work enqueued later:
 * with two windows, upload(i+1) overlaps the evaluation of window i.  Pass NULL for columns
 * the query does not read (range / join: x, y = 16 B per point; kNN: x, y, objID; ts is never
 * read by window evaluation).  Host buffers from gf_pinned_alloc copy asynchronously at PCIe
 * rate; pageable ones are staged by the runtime.
 * gf_window_points MUST be called after each upload and before the evaluation that reads the
 * window: it orders the context's streams after the copy.  Columns not uploaded come back
 * NULL (a kNN plan then reports GF_ERR_ARG). */
int  gf_window_create(gf_ctx* ctx, int64_t capacity, gf_window** out);
void gf_window_destroy(gf_window* w);
int  gf_window_upload(gf_window* w, const double* x, const double* y, const int64_t* objID,
                      const int64_t* ts, int64_t n);
int  gf_window_points(gf_window* w, gf_points* out);
/* kNN windows at 16 B per point over PCIe (HipKnnWindowFunction.java:96-106 hands x, y, objID):
 * x and y are copied as gf_window_upload does, but the objID column stays in host memory --
 * objID_pinned must be gf_pinned_alloc memory -- and the kernels read it in place through the
 * mapping: only the few hundred candidates' objIDs ever cross the bus (the scan appends
 * (d, idx, objID) for points below the threshold; nothing else reads objID).  The column must
 * stay unchanged until the work that reads this window has completed. */
int  gf_window_upload_mapped(gf_window* w, const double* x, const double* y, const int64_t* objID_pinned, int64_t n);
/* *pinned = 1 when p lies in pinned host memory (gf_pinned_alloc / registered), so a shim can
 * take gf_window_upload_mapped for an objID column it was handed. */
int  gf_host_pinned(const void* p, int* pinned);

/* ---- synthetic input (host) ----------------------------------------------------------
 * java.util.Random(seed): x = minX + nextDouble()*(maxX-minX), then y likewise, per point
 * (cf. SyntheticGpsSource.java:23,40-41). */
int gf_synth_uniform(int64_t seed, int64_t n, double minX, double maxX, double minY, double maxY,
                     double* x, double* y);

#ifdef __cplusplus
}
#endif
#endif /* GEOFLINK_HIP_H */
