"""Spatial operators -- mirrors of GeoFlink.spatialOperators.{range,knn,join} for one window.

The reference builds a Flink DAG per operator and evaluates each window inside a
WindowFunction.apply; here run() takes the window's points (a PointWindow, device SoA) and
evaluates that window on the GPU through the C ABI -- the body of apply() is what moved.

  PointPointRangeQuery.run(window, Set<Point>, r)     -- range/PointPointRangeQuery.java:37,111-187
  PointPolygonRangeQuery.run(window, Set<Polygon>, r) -- range/PointPolygonRangeQuery.java:31,134-205
  PointPointKNNQuery.run(window, Point, r, k)         -- knn/PointPointKNNQuery.java:33,132-201
  PointPointJoinQuery.run(ordinary, query, r)         -- join/PointPointJoinQuery.java:24,124-183
  PointPolygonJoinQuery.run(points, polygons, r)      -- join/PointPolygonJoinQuery.java:154-213
  PointLineStringRangeQuery.run(window, Set<LineString>, r) -- range/PointLineStringRangeQuery.java:100-172
  PointLineStringKNNQuery.run(window, LineString, r, k)     -- knn/PointLineStringKNNQuery.java (windowBased)
  PointLineStringJoinQuery.run(points, lineStrings, r)      -- join/PointLineStringJoinQuery.java (windowBased)
  {Polygon,LineString}{Point,Polygon,LineString}JoinQuery.run(ordinary, query, r)
                                                      -- join/*JoinQuery.java (windowBased): geometry windows joined

Errors follow the reference: unsupported query types raise ValueError ("Not yet support",
IllegalArgumentException), candidate layers <= 0 raise CandidateLayersError (System.exit(1)).
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from dataclasses import dataclass
from enum import Enum

import numpy as np

from . import _lib
from .spatialIndices import UniformGrid, generateCellIDStr
from .spatialObjects import (GeometryWindow, LineString, LineStringSet, LineStringWindow, Point, PointWindow, Polygon,
                             PolygonSet, PolygonWindow)


class QueryType(Enum):
    """QueryType.java:3-8"""
    RealTime = 0
    WindowBased = 1
    CountBased = 2
    RealTimeNaive = 3


class QueryConfiguration:
    """QueryConfiguration.java:5-57 (+ distanceMetric: JTS Coordinate.distance variant)."""

    def __init__(self, queryType: QueryType = None):
        self.queryType = queryType
        self.windowSize = 0
        self.slideStep = 0
        self.allowedLateness = 0
        self.approximateQuery = False
        self.distanceMetric = _lib.METRIC_SQRT

    def getQueryType(self): return self.queryType
    def setQueryType(self, t): self.queryType = t
    def getWindowSize(self): return self.windowSize
    def setWindowSize(self, v): self.windowSize = int(v)
    def getSlideStep(self): return self.slideStep
    def setSlideStep(self, v): self.slideStep = int(v)
    def getAllowedLateness(self): return self.allowedLateness
    def setAllowedLateness(self, v): self.allowedLateness = int(v)
    def isApproximateQuery(self): return self.approximateQuery
    def setApproximateQuery(self, v): self.approximateQuery = bool(v)


_SUPPORTED = (QueryType.RealTime, QueryType.WindowBased)


def _require_supported(conf: QueryConfiguration):
    # RealTime and WindowBased share the per-point semantics evaluated here (the RealTime
    # flatMap bodies equal the window apply bodies); the others throw in the reference too.
    if conf.getQueryType() not in _SUPPORTED:
        raise ValueError("Not yet support")


class _PlanCache:
    """Device plans of one operator, keyed by query CONTENTS (coordinates, polygon digest,
    radius, flags) and bounded: the least recently used plan beyond `limit` is destroyed, so a
    query stream (a new polygon set per window) does not leak one device plan per window."""

    def __init__(self, destroy_name: str, limit: int = 16):
        self._destroy_name = destroy_name
        self.limit = int(limit)
        self._d = OrderedDict()
        self._pinned = set()  # plans with state beyond their key (pipeline, capacity)
        self._held = {}       # plan -> number of pane engines (gf_*_sliding) borrowing it: never destroyed under them
        self._orphans = {}    # held plans of a closed cache: destroyed when their engine lets go

    def pin(self, plan):
        """Never evict `plan`: a plan with settings or pending pipelined work lives until it is
        unpinned or the operator closes."""
        self._pinned.add(self._pv(plan))

    def unpin(self, plan):
        """The plan is an ordinary LRU entry again and is evicted if the cache is over its limit."""
        self._pinned.discard(self._pv(plan))
        self._evict(None)

    def hold(self, plan):
        """A pane engine borrows `plan` (the engine dereferences it until it is destroyed): the
        plan is not evicted, and close() leaves its destruction to release() -- the operator and
        the engine may be finalized in either order (both die in one collected cycle).  Holds
        count: engines sharing one plan (two range engines on one query) each hold it, and it stays
        until the last of them lets go."""
        pv = self._pv(plan)
        self._held[pv] = self._held.get(pv, 0) + 1

    def holds(self, plan) -> int:
        """Number of pane engines borrowing `plan`."""
        return self._held.get(self._pv(plan), 0)

    def release(self, plan):
        """A pane engine is destroyed: once no engine holds the plan it is an ordinary LRU entry
        again, or, if the cache closed meanwhile, destroyed now."""
        pv = self._pv(plan)
        n = self._held.get(pv, 0)
        if n > 1:
            self._held[pv] = n - 1
            return
        self._held.pop(pv, None)
        orphan = self._orphans.pop(pv, None)
        if orphan is not None:
            self._destroy(orphan)
        else:
            self._evict(None)

    def get(self, key):
        plan = self._d.get(key)
        if plan is not None:
            self._d.move_to_end(key)
        return plan

    def put(self, key, plan):
        self._d[key] = plan
        self._evict(key)

    def _evict(self, keep):
        """Destroy least recently used unpinned plans beyond `limit`, never `keep` (the plan being
        inserted, which the caller is about to use): with `limit` pinned plans the cache simply
        grows past its limit until pins are released."""
        over = len(self._d) - self.limit
        if over <= 0:
            return
        victims = [k for k, p in self._d.items()
                   if k != keep and self._pv(p) not in self._pinned and self._pv(p) not in self._held][:over]
        for k in victims:
            self._destroy(self._d.pop(k))

    @staticmethod
    def _pv(plan):
        return plan.value if hasattr(plan, "value") else plan

    def _destroy(self, plan):
        if _lib._lib is not None:
            getattr(_lib._lib, self._destroy_name)(plan)

    def __len__(self):
        return len(self._d)

    def close(self):
        while self._d:
            _, p = self._d.popitem(last=False)
            if self._pv(p) in self._held:
                self._orphans[self._pv(p)] = p
            else:
                self._destroy(p)
        self._pinned.clear()


class SpatialOperator:
    _destroy_name = "gf_range_plan_destroy"

    def __init__(self, conf: QueryConfiguration, index: UniformGrid):
        self.conf = conf
        self.index = index
        self._plans = _PlanCache(self._destroy_name)

    def getQueryConfiguration(self):
        return self.conf

    def getSpatialIndex(self):
        return self.index


# ----------------------------------------------------------------------------------------
# range
# ----------------------------------------------------------------------------------------
@dataclass
class RangeResult:
    """Selection bitmap of one window (bit i = point i emitted) plus counts.

    For approximate point-point queries with |Q| > 1 the reference emits candidate-cell
    points once per query point: `multi` marks those points (multiplicity |Q|)."""

    window: PointWindow
    bitmap: object          # torch int64 [(n+63)/64] (uint64 words)
    counts: object          # torch int64 [2]: points emitted, multiset size
    multi: object = None
    nq: int = 1
    ctx: object = None

    def count(self) -> int:
        return int(self.counts[0].item())

    def multiset_size(self) -> int:
        return int(self.counts[1].item())

    def indices(self) -> np.ndarray:
        """Ascending indices of emitted points (each once)."""
        return bitmap_indices(self.ctx, self.bitmap, self.window.n)

    def multiset_indices(self) -> np.ndarray:
        idx = self.indices().astype(np.int64)
        if self.multi is None or self.nq <= 1:
            return idx
        m = bitmap_indices(self.ctx, self.multi, self.window.n).astype(np.int64)
        return np.sort(np.concatenate([idx] + [m] * (self.nq - 1)), kind="stable")

    def points(self, uGrid=None):
        return [self.window.point(i, uGrid) for i in self.indices()]


def bitmap_indices(ctx, bitmap, n) -> np.ndarray:
    import torch

    cap = max(1, int(n))
    out = torch.empty(cap, dtype=torch.int32, device=bitmap.device)
    cnt = C.c_int64()
    st = _lib.lib().gf_bitmap_to_indices(ctx.handle, bitmap.data_ptr(), int(n), out.data_ptr(), cap, C.byref(cnt))
    _lib.check(st, ctx.handle, "gf_bitmap_to_indices")
    return out[: cnt.value].cpu().numpy().view(np.uint32)


class _RangeBase(SpatialOperator):
    def _evaluate(self, plan, window: PointWindow, nq: int) -> RangeResult:
        import torch

        ctx = _lib.context(window.x.device.index)
        n = window.n
        words = max(1, (n + 63) // 64)
        bitmap = torch.empty(words, dtype=torch.int64, device=window.x.device)
        multi = torch.empty(words, dtype=torch.int64, device=window.x.device) if nq > 1 else None
        counts = torch.zeros(2, dtype=torch.int64, device=window.x.device)
        pts = window.c_struct()
        st = _lib.lib().gf_range_run(plan, C.byref(pts), bitmap.data_ptr(),
                                     multi.data_ptr() if multi is not None else None, counts.data_ptr())
        _lib.check(st, ctx.handle, "gf_range_run")
        return RangeResult(window, bitmap, counts, multi, nq, ctx)

    def _plan(self, key, create):
        plan = self._plans.get(key)
        if plan is None:
            plan = create()
            self._plans.put(key, plan)
            tuning = getattr(self, "tuning", None)  # (scan_blocks, defer_mode): gf_range_plan_set_tuning
            if tuning is not None:
                _lib.check(_lib.lib().gf_range_plan_set_tuning(plan, int(tuning[0]), int(tuning[1])), None,
                           "gf_range_plan_set_tuning")
            lanes = getattr(self, "drain_lanes", None)  # testing: gf_range_plan_set_drain_lanes
            if lanes is not None:
                _lib.check(_lib.lib().gf_range_plan_set_drain_lanes(plan, int(lanes)), None,
                           "gf_range_plan_set_drain_lanes")
        return plan

    def __del__(self):
        plans = getattr(self, "_plans", None)
        if plans is not None:
            plans.close()


class PointPointRangeQuery(_RangeBase):
    """range/PointPointRangeQuery.java -- window-based point-point range query."""

    def run(self, window: PointWindow, queryPointSet, queryRadius: float) -> RangeResult:
        _require_supported(self.conf)
        qs = list(queryPointSet)
        ctx, plan = self.plan(window.x.device.index, qs, queryRadius)
        nq = len(qs) if self.conf.approximateQuery else 1
        return self._evaluate(plan, window, nq)

    def plan(self, device: int, queryPointSet, queryRadius: float):
        """(context, gf_range_plan) of this query on `device` (cached by query contents)."""
        _require_supported(self.conf)
        qs = list(queryPointSet)
        qx = np.array([q.x for q in qs], np.float64)
        qy = np.array([q.y for q in qs], np.float64)
        ctx = _lib.context(device)
        key = (ctx.device, tuple(qx.tolist()), tuple(qy.tolist()), float(queryRadius),
               bool(self.conf.approximateQuery), int(self.conf.distanceMetric))

        def create():
            h = C.c_void_p()
            st = _lib.lib().gf_range_pp_plan_create(ctx.handle, C.byref(self.index.c_grid), qx.ctypes.data,
                                                    qy.ctypes.data, len(qs), float(queryRadius),
                                                    int(self.conf.approximateQuery), int(self.conf.distanceMetric),
                                                    C.byref(h))
            _lib.check(st, ctx.handle, "gf_range_pp_plan_create")
            return h

        return ctx, self._plan(key, create)


class PointPolygonRangeQuery(_RangeBase):
    """range/PointPolygonRangeQuery.java -- window-based point-polygon range query."""

    def run(self, window: PointWindow, queryPolygonSet, queryRadius: float) -> RangeResult:
        _require_supported(self.conf)
        ctx, plan = self.plan(window.x.device.index, queryPolygonSet, queryRadius)
        return self._evaluate(plan, window, 1)

    def plan(self, device: int, queryPolygonSet, queryRadius: float):
        """(context, gf_range_plan) of this query on `device` (cached by query contents)."""
        _require_supported(self.conf)
        ps = PolygonSet(queryPolygonSet)
        ctx = _lib.context(device)
        key = (ctx.device, ps.digest(), float(queryRadius), bool(self.conf.approximateQuery),
               int(self.conf.distanceMetric))

        def create():
            cs = ps.c_struct()
            h = C.c_void_p()
            st = _lib.lib().gf_range_ppoly_plan_create(ctx.handle, C.byref(self.index.c_grid), C.byref(cs),
                                                       float(queryRadius), int(self.conf.approximateQuery),
                                                       int(self.conf.distanceMetric), C.byref(h))
            _lib.check(st, ctx.handle, "gf_range_ppoly_plan_create")
            return h

        return ctx, self._plan(key, create)


def _linestring_plan(op, create_name, grid, device, lineStrings, queryRadius):
    """(context, plan, LineStringSet) of a linestring range / join plan of `op`, cached by the lines'
    contents; op.chain_mode (testing / tuning: 1 = the plain segment loop) is part of the key."""
    ls = lineStrings if isinstance(lineStrings, LineStringSet) else LineStringSet(lineStrings)
    ctx = _lib.context(device)
    mode = int(getattr(op, "chain_mode", 0))
    key = (create_name, ctx.device, ls.digest(), float(queryRadius), bool(op.conf.approximateQuery),
           int(op.conf.distanceMetric), mode)

    def create():
        cs = ls.c_struct()
        h = C.c_void_p()
        st = getattr(_lib.lib(), create_name)(ctx.handle, C.byref(grid.c_grid), C.byref(cs), float(queryRadius),
                                              int(op.conf.approximateQuery), int(op.conf.distanceMetric), C.byref(h))
        _lib.check(st, ctx.handle, create_name)
        if mode:
            _lib.check(_lib.lib().gf_range_plan_set_chain_mode(h, mode), ctx.handle, "gf_range_plan_set_chain_mode")
        return h

    return ctx, op._plan(key, create), ls


class PointLineStringRangeQuery(_RangeBase):
    """range/PointLineStringRangeQuery.java -- the point-polygon range query with the geometry renamed
    (windowBased :100-172; realTime :35-97 is the same per-point predicate): a point of a guaranteed
    cell is emitted, a point of a candidate cell if some line is within r -- Point.distance(LineString)
    (DistanceFunctions.java:38-42, the minimum of pointToSegment over the open chain, no containment)
    or, approximate, the bbox distance (:203-255)."""

    def run(self, window: PointWindow, queryLineStringSet, queryRadius: float) -> RangeResult:
        _require_supported(self.conf)
        ctx, plan = self.plan(window.x.device.index, queryLineStringSet, queryRadius)
        return self._evaluate(plan, window, 1)

    def plan(self, device: int, queryLineStringSet, queryRadius: float):
        """(context, gf_range_plan) of this query on `device` (cached by query contents)."""
        _require_supported(self.conf)
        ctx, plan, _ = _linestring_plan(self, "gf_range_pls_plan_create", self.index, device, queryLineStringSet,
                                        queryRadius)
        return ctx, plan


# ----------------------------------------------------------------------------------------
# kNN
# ----------------------------------------------------------------------------------------
@dataclass
class KNNResult:
    """Tuple3<winStart, winEnd, PriorityQueue<Tuple2<Point, Double>>> as sorted arrays:
    rank i = (objID[i], dist[i]), point index idx[i] in the window."""

    windowStart: int
    windowEnd: int
    objID: np.ndarray
    dist: np.ndarray
    idx: np.ndarray

    def __len__(self):
        return len(self.objID)

    def tuples(self):
        return list(zip(self.objID.tolist(), self.dist.tolist()))


def knn_record_bytes(k: int) -> int:
    return int(_lib.lib().gf_knn_result_bytes(int(k)))


def decode_knn_record(raw: bytes, k: int):
    """Decode a host copy of a device kNN record -> (status, objID, dist, idx)."""
    h = _lib.GfKnnHeader.from_buffer_copy(raw[: C.sizeof(_lib.GfKnnHeader)])
    off = C.sizeof(_lib.GfKnnHeader)
    d = np.frombuffer(raw, np.float64, k, off)
    o = np.frombuffer(raw, np.int64, k, off + 8 * k)
    i = np.frombuffer(raw, np.int64, k, off + 16 * k)
    return h.status, o[: h.n].copy(), d[: h.n].copy(), i[: h.n].copy()


class PinnedRecords:
    """A ring of kNN records in mapped pinned host memory (gf_pinned_alloc).  Pass
    `ptr(i)` as the record of enqueue(): the select kernel writes the record straight into
    host memory, so no copy kernel runs per window; read `raw(i)` after the stream syncs."""

    def __init__(self, count: int, k: int):
        self.k = int(k)
        self.count = int(count)
        self.bytes = knn_record_bytes(k)
        p = C.c_void_p()
        _lib.check(_lib.lib().gf_pinned_alloc(self.bytes * self.count, C.byref(p)), None, "gf_pinned_alloc")
        self._base = p.value
        self.view = np.ctypeslib.as_array((C.c_uint8 * (self.bytes * self.count)).from_address(self._base))
        self.view[:] = 0

    def ptr(self, i: int) -> int:
        return self._base + (i % self.count) * self.bytes

    def raw(self, i: int) -> bytes:
        j = i % self.count
        return self.view[j * self.bytes:(j + 1) * self.bytes].tobytes()

    def decode(self, i: int):
        return decode_knn_record(self.raw(i), self.k)

    def __del__(self):
        base = getattr(self, "_base", None)
        if base and _lib._lib is not None:
            self.view = None
            _lib._lib.gf_pinned_free(C.c_void_p(base))
            self._base = None


class PointPointKNNQuery(SpatialOperator):
    """knn/PointPointKNNQuery.java -- continuous kNN of one query point within radius r."""

    _destroy_name = "gf_knn_plan_destroy"

    def __init__(self, conf: QueryConfiguration, index: UniformGrid):
        super().__init__(conf, index)
        self._depth = {}  # plan handle -> pipeline depth (set_pipeline)

    @staticmethod
    def _pv(plan):
        return plan.value if hasattr(plan, "value") else plan

    def plan(self, window_device: int, queryPoint: Point, queryRadius: float, k: int):
        ctx = _lib.context(window_device)
        key = (ctx.device, queryPoint.x, queryPoint.y, float(queryRadius), int(k), int(self.conf.distanceMetric))
        plan = self._plans.get(key)
        if plan is None:
            h = C.c_void_p()
            st = _lib.lib().gf_knn_pp_plan_create(ctx.handle, C.byref(self.index.c_grid), float(queryPoint.x),
                                                  float(queryPoint.y), float(queryRadius), int(k),
                                                  int(self.conf.distanceMetric), C.byref(h))
            _lib.check(st, ctx.handle, "gf_knn_pp_plan_create")
            self._plans.put(key, h)
            plan = h
        return ctx, plan

    def run(self, window: PointWindow, queryPoint: Point, queryRadius: float, k: int) -> KNNResult:
        _require_supported(self.conf)
        if k is None or int(k) < 1:
            raise ValueError("k must be >= 1 (PriorityQueue initialCapacity < 1)")
        ctx, plan = self.plan(window.x.device.index, queryPoint, queryRadius, k)
        kk = int(k)
        oo = np.empty(kk, np.int64); od = np.empty(kk, np.float64); oi = np.empty(kk, np.int64)
        n = C.c_int32()
        pts = window.c_struct()
        st = _lib.lib().gf_knn_run(plan, C.byref(pts), oo.ctypes.data, od.ctypes.data, oi.ctypes.data, C.byref(n))
        _lib.check(st, ctx.handle, "gf_knn_run")
        m = n.value
        return KNNResult(window.start, window.end, oo[:m].copy(), od[:m].copy(), oi[:m].copy())

    def enqueue(self, window: PointWindow, queryPoint: Point, queryRadius: float, k: int, record):
        """Async: evaluate the window into a record -- a torch uint8 device tensor of
        knn_record_bytes(k), or an int address from PinnedRecords.ptr() (kernel writes the
        host record directly); pair with finish() once the record is on the host.  The window's
        tensors must stay alive until the record is complete (at depth >= 3 kernels on the plan's
        other streams read them, which torch's caching allocator does not track)."""
        ctx, plan = self.plan(window.x.device.index, queryPoint, queryRadius, k)
        pts = window.c_struct()
        addr = record if isinstance(record, int) else record.data_ptr()
        # depth >= 3 launches windows on the plan's other streams, which do not wait for the
        # context stream (torch's current stream, where this window's tensors were produced):
        # every enqueue orders those streams after it (gf_ctx_fork records one event), so a
        # window refilled in place on torch's stream is complete before any kernel reads it
        if self._depth.get(self._pv(plan), 1) >= 3:
            _lib.check(_lib.lib().gf_ctx_fork(ctx.handle), ctx.handle, "gf_ctx_fork")
        _lib.check(_lib.lib().gf_knn_enqueue(plan, C.byref(pts), C.c_void_p(addr)), ctx.handle, "gf_knn_enqueue")

    def finish(self, window: PointWindow, queryPoint: Point, queryRadius: float, k: int, raw: bytes) -> KNNResult:
        ctx, plan = self.plan(window.x.device.index, queryPoint, queryRadius, k)
        kk = int(k)
        oo = np.empty(kk, np.int64); od = np.empty(kk, np.float64); oi = np.empty(kk, np.int64)
        n = C.c_int32()
        buf = C.create_string_buffer(bytes(raw), len(raw))
        pts = window.c_struct()
        st = _lib.lib().gf_knn_decode(plan, C.byref(pts), buf, oo.ctypes.data, od.ctypes.data, oi.ctypes.data,
                                      C.byref(n))
        _lib.check(st, ctx.handle, "gf_knn_decode")
        m = n.value
        return KNNResult(window.start, window.end, oo[:m].copy(), od[:m].copy(), oi[:m].copy())

    def set_pipeline(self, window_device, queryPoint, queryRadius, k, depth: int):
        """depth 2: one fused launch per window; window i's record is written by the next
        enqueue (its select runs in block 0 of window i+1's scan) or by flush()."""
        ctx, plan = self.plan(window_device, queryPoint, queryRadius, k)
        _lib.check(_lib.lib().gf_knn_plan_set_pipeline(plan, int(depth)), ctx.handle, "set_pipeline")
        self._plans.pin(plan)  # its depth and pending records must survive the LRU
        self._depth[self._pv(plan)] = int(depth)

    def flush(self, window_device, queryPoint, queryRadius, k):
        ctx, plan = self.plan(window_device, queryPoint, queryRadius, k)
        _lib.check(_lib.lib().gf_knn_plan_flush(plan), ctx.handle, "flush")

    def set_capacity(self, window_device, queryPoint, queryRadius, k, cap):
        ctx, plan = self.plan(window_device, queryPoint, queryRadius, k)
        _lib.check(_lib.lib().gf_knn_plan_set_capacity(plan, int(cap)), ctx.handle, "set_capacity")
        self._plans.pin(plan)

    def __del__(self):
        plans = getattr(self, "_plans", None)
        if plans is not None:
            plans.close()


class PointPolygonKNNQuery(PointPointKNNQuery):
    """knn/PointPolygonKNNQuery.java -- continuous kNN of the window's points to one query
    polygon within r (JTS point-polygon distance, 0 inside; approximate: the bbox distance).
    Same run / enqueue / finish API as PointPointKNNQuery with a Polygon as the query."""

    def plan(self, window_device: int, queryPolygon: Polygon, queryRadius: float, k: int):
        ctx = _lib.context(window_device)
        ps = PolygonSet([queryPolygon])
        key = (ctx.device, ps.digest(), float(queryRadius), int(k), int(self.conf.distanceMetric),
               bool(self.conf.isApproximateQuery()))
        plan = self._plans.get(key)
        if plan is None:
            cs = ps.c_struct()
            h = C.c_void_p()
            st = _lib.lib().gf_knn_ppoly_plan_create(ctx.handle, C.byref(self.index.c_grid), C.byref(cs),
                                                     float(queryRadius), int(k), int(self.conf.isApproximateQuery()),
                                                     int(self.conf.distanceMetric), C.byref(h))
            _lib.check(st, ctx.handle, "gf_knn_ppoly_plan_create")
            self._plans.put(key, h)
            plan = h
        return ctx, plan


class PointLineStringKNNQuery(PointPointKNNQuery):
    """knn/PointLineStringKNNQuery.java (windowBased, then KNNQuery.kNNWinAllEvaluationPointStream) --
    continuous kNN of the window's points to one query linestring within r: candidates have their cell
    in C u G of the line's bbox cells and d <= r, d = the open-chain distance (no containment) or,
    approximate, the bbox distance.  The polygon query's record contract and run / enqueue / finish API
    with a LineString as the query.  chain_mode = 1 (testing / tuning) runs the plain segment loop."""

    chain_mode = 0

    def plan(self, window_device: int, queryLineString: LineString, queryRadius: float, k: int):
        ctx = _lib.context(window_device)
        ls = LineStringSet([queryLineString])
        mode = int(self.chain_mode)
        key = (ctx.device, ls.digest(), float(queryRadius), int(k), int(self.conf.distanceMetric),
               bool(self.conf.isApproximateQuery()), mode)
        plan = self._plans.get(key)
        if plan is None:
            cs = ls.c_struct()
            h = C.c_void_p()
            st = _lib.lib().gf_knn_pls_plan_create(ctx.handle, C.byref(self.index.c_grid), C.byref(cs),
                                                   float(queryRadius), int(k), int(self.conf.isApproximateQuery()),
                                                   int(self.conf.distanceMetric), C.byref(h))
            _lib.check(st, ctx.handle, "gf_knn_pls_plan_create")
            if mode:
                _lib.check(_lib.lib().gf_knn_plan_set_chain_mode(h, mode), ctx.handle, "gf_knn_plan_set_chain_mode")
            self._plans.put(key, h)
            plan = h
        return ctx, plan


def knn_merge_host(k: int, lists):
    """Top-k distinct objIDs of several sorted (objID, dist, idx) lists -- the windowAll funnel
    (KNNQuery.java:213-272) across shards; host code of the library (no GPU needed)."""
    counts = np.array([len(l[0]) for l in lists], np.int32)
    o = np.ascontiguousarray(np.concatenate([np.asarray(l[0], np.int64) for l in lists]) if lists else
                             np.zeros(0, np.int64))
    d = np.ascontiguousarray(np.concatenate([np.asarray(l[1], np.float64) for l in lists]) if lists else
                             np.zeros(0, np.float64))
    i = np.ascontiguousarray(np.concatenate([np.asarray(l[2], np.int64) for l in lists]) if lists else
                             np.zeros(0, np.int64))
    oo = np.empty(k, np.int64); od = np.empty(k, np.float64); oi = np.empty(k, np.int64)
    n = C.c_int32()
    st = _lib.lib().gf_knn_merge_host(int(k), len(lists), counts.ctypes.data, o.ctypes.data, d.ctypes.data,
                                      i.ctypes.data, oo.ctypes.data, od.ctypes.data, oi.ctypes.data, C.byref(n))
    _lib.check(st, None, "gf_knn_merge_host")
    return oo[: n.value].copy(), od[: n.value].copy(), oi[: n.value].copy()


# ----------------------------------------------------------------------------------------
# join
# ----------------------------------------------------------------------------------------
class PointPointJoinQuery(SpatialOperator):
    """join/PointPointJoinQuery.java -- window-based point-point join.  index1 = uGrid
    (ordinary stream), index2 = qGrid (query stream, replicated to neighbour cells)."""

    def __init__(self, conf: QueryConfiguration, index1: UniformGrid, index2: UniformGrid = None):
        super().__init__(conf, index1)
        self.index2 = index2 if index2 is not None else index1

    def run(self, ordinaryWindow: PointWindow, queryWindow: PointWindow, queryRadius: float) -> np.ndarray:
        """Returns int64 [m, 2] pairs (ordinary index, query index), sorted."""
        import torch

        _require_supported(self.conf)
        ctx = _lib.context(ordinaryWindow.x.device.index)
        po, pq = ordinaryWindow.c_struct(), queryWindow.c_struct()
        cap = max(1024, 4 * (ordinaryWindow.n + queryWindow.n))
        for _ in range(2):
            pairs = torch.empty(2 * cap, dtype=torch.int32, device=ordinaryWindow.x.device)
            npairs = C.c_int64()
            st = _lib.lib().gf_join_pp(ctx.handle, C.byref(self.index.c_grid), C.byref(self.index2.c_grid),
                                       C.byref(po), C.byref(pq), float(queryRadius), int(self.conf.approximateQuery),
                                       int(self.conf.distanceMetric), pairs.data_ptr(), cap, C.byref(npairs))
            if st == _lib.GF_ERR_CAPACITY:
                cap = int(npairs.value)
                continue
            _lib.check(st, ctx.handle, "gf_join_pp")
            m = int(npairs.value)
            out = pairs[: 2 * m].cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 2)
            order = np.lexsort((out[:, 1], out[:, 0]))
            return out[order]
        raise _lib.GeoFlinkError(_lib.GF_ERR_CAPACITY, "join output kept growing")


class PointPolygonJoinQuery(_RangeBase):
    """join/PointPolygonJoinQuery.java -- window-based join of a point stream with a polygon
    stream (PointPolygonJoinQuery.java:154-213; polygons replicated to their own guaranteed +
    candidate cells, JoinQuery.java:93-115).  index1 = uGrid (points), index2 = qGrid
    (polygons); the device path requires the two grids to be equal.  The replicated polygon
    side is a plan, cached by the polygons' contents (a static query set reuses it; a polygon
    stream's window with new geometry builds a new one, the cache keeps the 16 most recent)."""

    def __init__(self, conf: QueryConfiguration, index1: UniformGrid, index2: UniformGrid = None):
        super().__init__(conf, index1)
        self.index2 = index2 if index2 is not None else index1

    def run(self, pointWindow: PointWindow, queryPolygons, queryRadius: float) -> np.ndarray:
        """Returns int64 [m, 2] pairs (point index, polygon index), sorted."""
        import torch

        _require_supported(self.conf)
        ps = PolygonSet(queryPolygons)  # keeps the CSR arrays alive during the call
        ctx = _lib.context(pointWindow.x.device.index)
        key = (ctx.device, ps.digest(), float(queryRadius), bool(self.conf.approximateQuery),
               int(self.conf.distanceMetric))

        def create():
            cs = ps.c_struct()
            h = C.c_void_p()
            _lib.check(_lib.lib().gf_join_ppoly_plan_create(ctx.handle, C.byref(self.index2.c_grid), C.byref(cs),
                                                            float(queryRadius), int(self.conf.approximateQuery),
                                                            int(self.conf.distanceMetric), C.byref(h)),
                       ctx.handle, "gf_join_ppoly_plan_create")
            return h

        plan = self._plan(key, create)
        pts = pointWindow.c_struct()
        cap = max(1024, 2 * pointWindow.n)
        for _ in range(2):
            pairs = torch.empty(2 * cap, dtype=torch.int32, device=pointWindow.x.device)
            npairs = C.c_int64()
            st = _lib.lib().gf_join_ppoly_run(plan, C.byref(self.index.c_grid), C.byref(pts), pairs.data_ptr(), cap,
                                              C.byref(npairs))
            if st == _lib.GF_ERR_CAPACITY:
                cap = int(npairs.value)
                continue
            _lib.check(st, ctx.handle, "gf_join_ppoly_run")
            m = int(npairs.value)
            out = pairs[: 2 * m].cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 2)
            order = np.lexsort((out[:, 1], out[:, 0]))
            return out[order]
        raise _lib.GeoFlinkError(_lib.GF_ERR_CAPACITY, "join output kept growing")


class PointLineStringJoinQuery(_RangeBase):
    """join/PointLineStringJoinQuery.java (windowBased) -- window-based join of a point stream with a
    linestring stream: line q is replicated to its own guaranteed + candidate cells
    (JoinQuery.getReplicatedLineStringQueryStream, JoinQuery.java:117-137), point p pairs with q when
    their cells match and either the query is approximate or the open-chain distance is <= r.  The
    replicated side is a plan cached by the lines' contents, run by gf_join_ppoly_run; the device path
    requires the two grids to be equal, as PointPolygonJoinQuery does."""

    def __init__(self, conf: QueryConfiguration, index1: UniformGrid, index2: UniformGrid = None):
        super().__init__(conf, index1)
        self.index2 = index2 if index2 is not None else index1

    def run(self, pointWindow: PointWindow, queryLineStrings, queryRadius: float) -> np.ndarray:
        """Returns int64 [m, 2] pairs (point index, line index), sorted."""
        import torch

        _require_supported(self.conf)
        ctx, plan, _ls = _linestring_plan(self, "gf_join_pls_plan_create", self.index2, pointWindow.x.device.index,
                                          queryLineStrings, queryRadius)
        pts = pointWindow.c_struct()
        cap = max(1024, 2 * pointWindow.n)
        for _ in range(2):
            pairs = torch.empty(2 * cap, dtype=torch.int32, device=pointWindow.x.device)
            npairs = C.c_int64()
            st = _lib.lib().gf_join_ppoly_run(plan, C.byref(self.index.c_grid), C.byref(pts), pairs.data_ptr(), cap,
                                              C.byref(npairs))
            if st == _lib.GF_ERR_CAPACITY:
                cap = int(npairs.value)
                continue
            _lib.check(st, ctx.handle, "gf_join_ppoly_run")
            m = int(npairs.value)
            out = pairs[: 2 * m].cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 2)
            order = np.lexsort((out[:, 1], out[:, 0]))
            return out[order]
        raise _lib.GeoFlinkError(_lib.GF_ERR_CAPACITY, "join output kept growing")


# ----------------------------------------------------------------------------------------
# cell assignment / bucketing (the ingest-side pieces of the path)
# ----------------------------------------------------------------------------------------
def assign_cells(window: PointWindow, grid: UniformGrid):
    """K1: HelperClass.assignGridCellID for every point -> (cx, cy) int32 torch tensors."""
    import torch

    ctx = _lib.context(window.x.device.index)
    n = window.n
    cx = torch.empty(max(n, 1), dtype=torch.int32, device=window.x.device)
    cy = torch.empty(max(n, 1), dtype=torch.int32, device=window.x.device)
    pts = window.c_struct()
    _lib.check(_lib.lib().gf_assign_cells(ctx.handle, C.byref(grid.c_grid), C.byref(pts), cx.data_ptr(),
                                          cy.data_ptr()), ctx.handle, "gf_assign_cells")
    return cx[:n], cy[:n]


def bucket_by_cell(window: PointWindow, grid: UniformGrid):
    """K2: keyBy(gridID) analogue -> (perm, cell_start) with bucket n*n = out-of-grid."""
    import torch

    ctx = _lib.context(window.x.device.index)
    n = window.n
    g = grid.getNumGridPartitions()
    perm = torch.empty(max(n, 1), dtype=torch.int32, device=window.x.device)
    start = torch.empty(g * g + 2, dtype=torch.int32, device=window.x.device)
    pts = window.c_struct()
    _lib.check(_lib.lib().gf_bucket_by_cell(ctx.handle, C.byref(grid.c_grid), C.byref(pts), perm.data_ptr(),
                                            start.data_ptr()), ctx.handle, "gf_bucket_by_cell")
    return perm[:n], start


def synthetic_uniform(seed: int, n: int, minX: float, maxX: float, minY: float, maxY: float):
    """java.util.Random(seed)-compatible uniform points (SyntheticGpsSource.java:23,40-41)."""
    x = np.empty(n, np.float64)
    y = np.empty(n, np.float64)
    _lib.check(_lib.lib().gf_synth_uniform(int(seed), int(n), float(minX), float(maxX), float(minY), float(maxY),
                                           x.ctypes.data, y.ctypes.data), None, "gf_synth_uniform")
    return x, y


def synthetic_clustered(seed: int, n: int, minX: float, maxX: float, minY: float, maxY: float, centers=None,
                        n_centers: int = 8, sigma: float = 0.01, frac: float = 0.8):
    """The clustered variant of the synthetic source: a fraction `frac`
    of the points from Gaussian hot spots N(centre, sigma^2) (sigma in degrees), the rest
    uniform; `centers` (list of (x, y)) come first, the remaining of `n_centers` are uniform in
    the bounds.  Points falling outside the bounds are drawn again, so every point is inside.
    numpy PCG64(seed): deterministic, host-side (input generation, not the evaluated path)."""
    rng = np.random.default_rng(seed)
    cs = [tuple(c) for c in (centers or [])][:n_centers]
    while len(cs) < n_centers:
        cs.append((rng.uniform(minX, maxX), rng.uniform(minY, maxY)))
    cx = np.array([c[0] for c in cs], np.float64)
    cy = np.array([c[1] for c in cs], np.float64)
    x = np.empty(n, np.float64)
    y = np.empty(n, np.float64)
    todo = np.arange(n)
    while len(todo):
        m = len(todo)
        hot = rng.random(m) < frac
        k = rng.integers(0, len(cs), m)
        xv = np.where(hot, cx[k] + sigma * rng.standard_normal(m), rng.uniform(minX, maxX, m))
        yv = np.where(hot, cy[k] + sigma * rng.standard_normal(m), rng.uniform(minY, maxY, m))
        ok = (xv >= minX) & (xv < maxX) & (yv >= minY) & (yv < maxY)
        x[todo[ok]] = xv[ok]
        y[todo[ok]] = yv[ok]
        todo = todo[~ok]
    return x, y


# ----------------------------------------------------------------------------------------
# trajectories (the reference's t* operators: a window as the points of each objID in arrival order)
# ----------------------------------------------------------------------------------------
class TrajectoryGroups:
    """gf_traj_groups of one window: the window grouped by objID on the device (stable, trajectories
    in first-occurrence order).  regroup(window) reuses the device workspace for the next window."""

    def __init__(self, window: PointWindow):
        self.handle = C.c_void_p()
        self.regroup(window)

    def regroup(self, window: PointWindow):
        self.window = window
        self.ctx = _lib.context(window.x.device.index)
        pts = window.c_struct()
        _lib.check(_lib.lib().gf_traj_group(self.ctx.handle, C.byref(pts), C.byref(self.handle)), self.ctx.handle,
                   "gf_traj_group")
        nt, n = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().gf_traj_groups_info(self.handle, C.byref(nt), C.byref(n)), None, "gf_traj_groups_info")
        self.ntraj, self.n = nt.value, n.value
        return self

    def set_long_threshold(self, length: int):
        """Testing / tuning: trajectories of at least `length` points take tStats' block path (0: default)."""
        _lib.check(_lib.lib().gf_traj_groups_set_long_threshold(self.handle, int(length)), None,
                   "gf_traj_groups_set_long_threshold")

    def read(self):
        """(keys int64[ntraj], seg_off int64[ntraj + 1], perm uint32[n]) on the host."""
        keys = np.empty(self.ntraj, np.int64)
        off = np.empty(self.ntraj + 1, np.int64)
        perm = np.empty(self.n, np.uint32)
        _lib.check(_lib.lib().gf_traj_groups_read(self.handle, keys.ctypes.data, off.ctypes.data, perm.ctypes.data),
                   self.ctx.handle, "gf_traj_groups_read")
        return keys, off, perm

    def tstats(self, trajIDSet=(), cap=None):
        """(count, keys, spatialLength, temporalLength, speed): at most `cap` rows (default: all)."""
        ids = np.ascontiguousarray(np.asarray(list(trajIDSet), np.int64))
        cap = self.ntraj if cap is None else int(cap)
        keys, S, T, V = (np.empty(cap, np.int64), np.empty(cap, np.float64), np.empty(cap, np.int64),
                         np.empty(cap, np.float64))
        cnt = C.c_int64()
        pts = self.window.c_struct()
        st = _lib.lib().gf_tstats_run(self.handle, C.byref(pts), ids.ctypes.data if len(ids) else None, len(ids),
                                      keys.ctypes.data, S.ctypes.data, T.ctypes.data, V.ctypes.data, cap, C.byref(cnt))
        _lib.check(st, self.ctx.handle, "gf_tstats_run")
        m = min(cnt.value, cap)
        return cnt.value, keys[:m], S[:m], T[:m], V[:m]

    def select(self, bitmap):
        """Sub-trajectories of a device hit bitmap (torch int64 words) -> SubTrajectories."""
        pts = self.window.c_struct()
        return self._emit(lambda *a: _lib.lib().gf_traj_select(self.handle, C.byref(pts), bitmap.data_ptr() if self.n else None,
                                                               *a), "gf_traj_select")

    def _emit(self, call, name, cap_traj=None, cap_pts=None):
        """Host arrays of a gf_traj_select-shaped call -> SubTrajectories (at most cap_traj / cap_pts
        written; `totals` = the full counts)."""
        nt = self.ntraj if cap_traj is None else int(cap_traj)
        n = self.n if cap_pts is None else int(cap_pts)
        keys, off = np.empty(nt, np.int64), np.zeros(nt + 1, np.int64)
        x, y, ts, idx = np.empty(n, np.float64), np.empty(n, np.float64), np.empty(n, np.int64), np.empty(n, np.uint32)
        m, npts = C.c_int64(), C.c_int64()
        st = call(keys.ctypes.data, off.ctypes.data, nt, x.ctypes.data, y.ctypes.data, ts.ctypes.data, idx.ctypes.data, n,
                  C.byref(m), C.byref(npts))
        _lib.check(st, self.ctx.handle, name)
        k, q = min(m.value, nt), min(npts.value, n)
        out = SubTrajectories(self.window, keys[:k], off[:k + 1], x[:q], y[:q], ts[:q], idx[:q])
        out.totals = (m.value, npts.value)
        return out

    def trange(self, grid: UniformGrid, polygons, plan: "TRangePlan" = None, cap_traj=None, cap_pts=None) -> "SubTrajectories":
        """gf_trange_run: the trajectories of this grouped window with a point CONTAINED (JTS contains:
        located INTERIOR; a point on an edge is not) by some polygon, each whole.  plan: a TRangePlan of
        (grid, polygons) to reuse (default: one is built for the call and destroyed)."""
        own = plan is None
        if own:
            plan = TRangePlan(self.ctx, grid, polygons)
        try:
            pts = self.window.c_struct()
            return self._emit(lambda *a: _lib.lib().gf_trange_run(plan.handle, self.handle, C.byref(pts), *a), "gf_trange_run",
                              cap_traj, cap_pts)
        finally:
            if own:
                plan.close()

    def tfilter(self, trajIDSet=(), cap_traj=None, cap_pts=None) -> "SubTrajectories":
        """gf_tfilter_run: the trajectories whose objID key is in trajIDSet (keys), each whole; an empty
        set = every trajectory (PointTFilterQuery.java:92-95)."""
        ids = np.ascontiguousarray(np.asarray(list(trajIDSet), np.int64))
        pts = self.window.c_struct()
        return self._emit(lambda *a: _lib.lib().gf_tfilter_run(self.handle, C.byref(pts), ids.ctypes.data if len(ids) else None,
                                                               len(ids), *a), "gf_tfilter_run", cap_traj, cap_pts)

    def tknn(self, grid: UniformGrid, queryPoint, queryRadius: float, k: int, naive: bool = False, big_cell=None,
             cap_rows=None, cap_pts=None) -> "TKNNResult":
        """gf_tknn_run over this grouped window (PointPointTKNNQuery.run / runNaive without grouping the
        window again).  The gf_tknn object is kept and reused by later calls.  big_cell: the testing
        threshold of gf_tknn_set_thresholds (0: the default); cap_rows / cap_pts: read at most that many
        rows / points (default: all).  The result carries `info`: rows, npts, in_cells, pairs, records."""
        if getattr(self, "_tknn", None) is None:
            self._tknn = C.c_void_p()
        L = _lib.lib()
        if big_cell is not None and not self._tknn:
            raise ValueError("big_cell needs an earlier tknn() call on these groups")
        if big_cell is not None:
            _lib.check(L.gf_tknn_set_thresholds(self._tknn, int(big_cell)), None, "gf_tknn_set_thresholds")
        pts = self.window.c_struct()
        st = L.gf_tknn_run(self.handle, C.byref(grid.c_grid), C.byref(pts), float(queryPoint.x), float(queryPoint.y),
                           float(queryRadius), int(k), _lib.TKNN_NAIVE if naive else _lib.TKNN_GRID, C.byref(self._tknn))
        _lib.check(st, self.ctx.handle, "gf_tknn_run")
        c = [C.c_int64() for _ in range(5)]
        _lib.check(L.gf_tknn_info(self._tknn, *(C.byref(v) for v in c)), None, "gf_tknn_info")
        info = dict(zip(("rows", "npts", "in_cells", "pairs", "records"), (v.value for v in c)))
        m = info["rows"] if cap_rows is None else min(info["rows"], int(cap_rows))
        q = info["npts"] if cap_pts is None else min(info["npts"], int(cap_pts))
        keys, dist, cells, off = np.empty(m, np.int64), np.empty(m, np.float64), np.empty(m, np.int32), np.zeros(m + 1, np.int64)
        x, y, ts, idx = np.empty(q, np.float64), np.empty(q, np.float64), np.empty(q, np.int64), np.empty(q, np.uint32)
        st = L.gf_tknn_read(self._tknn, keys.ctypes.data, dist.ctypes.data, cells.ctypes.data, off.ctypes.data, m,
                            x.ctypes.data, y.ctypes.data, ts.ctypes.data, idx.ctypes.data, q)
        _lib.check(st, self.ctx.handle, "gf_tknn_read")
        return TKNNResult(self.window, keys, dist, cells, off, x, y, ts, idx, info)

    def tjoin(self, other: "TrajectoryGroups", grid: UniformGrid, r: float, single: bool = False,
              table_slots=None) -> "TJoinResult":
        """gf_tjoin_run: this grouped window as the ordinary side against `other`, the grouped query
        window (PointPointTJoinQuery.run), or against itself (single=True, runSingle: `other` is these
        groups).  The gf_tjoin object is kept and reused by later calls.  table_slots: the testing hook
        of gf_tjoin_set_table_slots (the first table size of this call; 0: the default).  The result
        carries `info`: rows, emitted, otraj, opoints, qtraj, qpoints, probe_passes."""
        L = _lib.lib()
        if getattr(self, "_tjoin", None) is None:
            self._tjoin = C.c_void_p()
        if table_slots is not None:
            if not self._tjoin:
                raise ValueError("table_slots needs an earlier tjoin() call on these groups")
            _lib.check(L.gf_tjoin_set_table_slots(self._tjoin, int(table_slots)), None, "gf_tjoin_set_table_slots")
        po, pq = self.window.c_struct(), other.window.c_struct()
        st = L.gf_tjoin_run(self.handle, C.byref(po), other.handle, C.byref(pq), C.byref(grid.c_grid), float(r),
                            _lib.TJOIN_SINGLE if single else _lib.TJOIN_PAIR, C.byref(self._tjoin))
        _lib.check(st, self.ctx.handle, "gf_tjoin_run")
        c = [C.c_int64() for _ in range(7)]
        _lib.check(L.gf_tjoin_info(self._tjoin, *(C.byref(v) for v in c)), None, "gf_tjoin_info")
        info = dict(zip(("rows", "emitted", "otraj", "opoints", "qtraj", "qpoints", "probe_passes"), (v.value for v in c)))
        m = info["rows"]
        okey, qkey = np.empty(m, np.int64), np.empty(m, np.int64)
        p_first, q_latest = np.empty(m, np.uint32), np.empty(m, np.uint32)
        emit, oslot, qslot = np.empty(m, np.uint8), np.empty(m, np.int32), np.empty(m, np.int32)
        st = L.gf_tjoin_read_rows(self._tjoin, okey.ctypes.data, qkey.ctypes.data, p_first.ctypes.data, q_latest.ctypes.data,
                                  emit.ctypes.data, oslot.ctypes.data, qslot.ctypes.data, m)
        _lib.check(st, self.ctx.handle, "gf_tjoin_read_rows")
        sides = []
        for side, (w, nt, npt) in enumerate(((self.window, info["otraj"], info["opoints"]),
                                             (other.window, info["qtraj"], info["qpoints"]))):
            keys, off = np.empty(nt, np.int64), np.zeros(nt + 1, np.int64)
            x, y, ts, idx = np.empty(npt, np.float64), np.empty(npt, np.float64), np.empty(npt, np.int64), np.empty(npt, np.uint32)
            st = L.gf_tjoin_read_trajs(self._tjoin, side, keys.ctypes.data, off.ctypes.data, nt, x.ctypes.data, y.ctypes.data,
                                       ts.ctypes.data, idx.ctypes.data, npt)
            _lib.check(st, self.ctx.handle, "gf_tjoin_read_trajs")
            sides.append(SubTrajectories(w, keys, off, x, y, ts, idx))
        return TJoinResult(okey, qkey, p_first, q_latest, emit.astype(bool), oslot, qslot, sides[0], sides[1], info)

    def close(self):
        t = getattr(self, "_tknn", None)
        if t and _lib._lib is not None:
            _lib._lib.gf_tknn_destroy(t)
            self._tknn = None
        t = getattr(self, "_tjoin", None)
        if t and _lib._lib is not None:
            _lib._lib.gf_tjoin_destroy(t)
            self._tjoin = None
        h = getattr(self, "handle", None)
        if h and _lib._lib is not None:
            _lib._lib.gf_traj_groups_destroy(h)
            self.handle = C.c_void_p()

    __del__ = close


@dataclass
class TStatsResult:
    """TStatsQuery's rows Tuple4<objID, spatialLength, temporalLength, speed> (TStatsQuery.java:186-188)
    as arrays, trajectories in first-occurrence order; objID holds the keys."""

    window: PointWindow
    objID: np.ndarray
    spatialLength: np.ndarray
    temporalLength: np.ndarray
    speed: np.ndarray

    def __len__(self):
        return len(self.objID)

    def objid_strings(self):
        """The rows' objID Strings, through the window's dictionary."""
        return self.window.objid_strings(self.objID)

    def tuples(self):
        return list(zip(self.objid_strings(), self.spatialLength.tolist(), self.temporalLength.tolist(),
                        self.speed.tolist()))


@dataclass
class SubTrajectories:
    """CSR of whole trajectories: trajectory j = objID[j], points [off[j], off[j+1]) of x, y, ts, idx
    (idx = index in the window), in arrival order; trajectories in first-occurrence order."""

    window: PointWindow
    objID: np.ndarray
    off: np.ndarray
    x: np.ndarray
    y: np.ndarray
    ts: np.ndarray
    idx: np.ndarray

    def __len__(self):
        return len(self.objID)

    def objid_strings(self):
        return self.window.objid_strings(self.objID)


class PointTStatsQuery:
    """tStats/PointTStatsQuery.java + TStatsQuery.java:148-189 -- window-based trajectory statistics:
    per objID, over its points in arrival order, the travelled length, the time it took and their
    quotient.  trajIDSet (objID Strings or keys; PointTStatsQuery.java:76-84): non-empty = only those."""

    def __init__(self, conf: QueryConfiguration, index: UniformGrid = None):
        self.conf = conf
        self.index = index

    def run(self, window: PointWindow, trajIDSet=()) -> TStatsResult:
        if self.conf.getQueryType() != QueryType.WindowBased:
            raise ValueError("Not yet support")
        ids = _traj_id_keys(window, trajIDSet)
        if ids is not None and len(ids) == 0:  # a non-empty set none of whose Strings the window can hold
            e = np.empty(0)
            return TStatsResult(window, e.astype(np.int64), e, e.astype(np.int64), e.copy())
        g = TrajectoryGroups(window)
        try:
            _, keys, S, T, V = g.tstats(() if ids is None else ids)
        finally:
            g.close()
        return TStatsResult(window, keys, S, T, V)


def _traj_id_keys(window: PointWindow, trajIDSet):
    """trajIDSet -> objID keys (None: no filter).  ints are keys; Strings are canonical decimals (their
    value) or looked up among the window's own objID Strings (a String the window does not hold
    cannot match and is dropped, never interned)."""
    items = list(trajIDSet)
    if not items:
        return None
    keys, strs = [], []
    for it in items:
        if isinstance(it, (int, np.integer)):
            keys.append(int(it))
        elif it is None:
            keys.append(_lib.OBJID_NULL)
        else:
            v = _canonical_decimal(str(it))
            if v is not None:
                keys.append(v)
            else:
                strs.append(str(it))
    if strs:
        uk = np.unique(window.objID.cpu().numpy())
        uk = uk[uk < _lib.OBJID_NUMERIC_MIN]
        if len(uk):
            want = set(strs)
            keys += [int(k) for k, s in zip(uk.tolist(), window.objid_strings(uk)) if s in want]
    return np.asarray(keys, np.int64)


def _canonical_decimal(s: str):
    """The key of a String that is exactly Long.toString(v), v in the numeric key range; else None."""
    try:
        v = int(s)
    except ValueError:
        return None
    return v if str(v) == s and _lib.OBJID_NUMERIC_MIN <= v < _lib.OBJID_NUMERIC_END else None


def group_by_objid(window: PointWindow):
    """The window grouped by objID: (keys[ntraj], seg_off[ntraj + 1], perm[n]) -- trajectory t is
    objID keys[t], its points perm[seg_off[t] : seg_off[t + 1]] in arrival order; trajectories in
    first-occurrence order."""
    g = TrajectoryGroups(window)
    try:
        return g.read()
    finally:
        g.close()


def sub_trajectories(window: PointWindow, hits) -> SubTrajectories:
    """Every trajectory with a hit point, whole (the assembly of the window-based tRange / tKnn /
    tJoin).  hits: a RangeResult of `window`, or a device bitmap (torch int64 words, bit i = point i)."""
    bitmap = hits.bitmap if isinstance(hits, RangeResult) else hits
    g = TrajectoryGroups(window)
    try:
        return g.select(bitmap)
    finally:
        g.close()


# ----------------------------------------------------------------------------------------
# tRange / tFilter (trajectories that enter a polygon set; trajectories of an id set)
# ----------------------------------------------------------------------------------------
class TRangePlan:
    """gf_trange_plan of (grid, polygon set) on one context: built once per continuous query."""

    def __init__(self, ctx, grid: UniformGrid, polygons):
        self.ctx = ctx
        self._owned = True
        ps = polygons if isinstance(polygons, PolygonSet) else PolygonSet(polygons)
        cs = ps.c_struct()
        self.handle = C.c_void_p()
        st = _lib.lib().gf_trange_plan_create(ctx.handle, C.byref(grid.c_grid), C.byref(cs), C.byref(self.handle))
        _lib.check(st, ctx.handle, "gf_trange_plan_create")

    def stats(self) -> dict:
        c = [C.c_int64() for _ in range(5)]
        _lib.check(_lib.lib().gf_trange_plan_stats(self.handle, *(C.byref(v) for v in c)), None, "gf_trange_plan_stats")
        return dict(zip(("none_cells", "test_cells", "inside_cells", "list_entries", "wide_polygons"), (v.value for v in c)))

    def set_thresholds(self, wide_ring: int = 0):
        """Testing / tuning: polygons whose largest ring has at least `wide_ring` vertices are tested by a
        wave per (point, polygon) (0: the default).  Results are identical for any value."""
        _lib.check(_lib.lib().gf_trange_plan_set_thresholds(self.handle, int(wide_ring)), self.ctx.handle,
                   "gf_trange_plan_set_thresholds")

    def info(self) -> dict:
        c = [C.c_int64() for _ in range(4)]
        _lib.check(_lib.lib().gf_trange_info(self.handle, *(C.byref(v) for v in c)), None, "gf_trange_info")
        return dict(zip(("cell_points", "inside_points", "wide_ring", "wave_path"), (v.value for v in c)))

    def points(self, window: PointWindow) -> RangeResult:
        """gf_trange_points: the contained points of `window` as a RangeResult (bitmap + count)."""
        import torch

        words = max(1, (window.n + 63) // 64)
        bitmap = torch.zeros(words, dtype=torch.int64, device=window.x.device)
        counts = torch.zeros(2, dtype=torch.int64, device=window.x.device)
        pts = window.c_struct()
        st = _lib.lib().gf_trange_points(self.handle, C.byref(pts), bitmap.data_ptr(), counts.data_ptr())
        _lib.check(st, self.ctx.handle, "gf_trange_points")
        return RangeResult(window, bitmap, counts, None, 1, self.ctx)

    def close(self):
        h = getattr(self, "handle", None)
        if h and getattr(self, "_owned", False) and _lib._lib is not None:
            _lib._lib.gf_trange_plan_destroy(h)
            self.handle = C.c_void_p()

    __del__ = close


class PointPolygonTRangeQuery(SpatialOperator):
    """tRange/PointPolygonTRangeQuery.java.  WindowBased (:89-176): the trajectories with a point contained
    by some polygon of the set, each whole -> SubTrajectories.  RealTime (:53-87): the contained points
    -> RangeResult.  contains is JTS's: a point on a shell or hole edge is not contained.  Plans are
    cached by the polygon set's digest."""

    _destroy_name = "gf_trange_plan_destroy"

    def plan(self, device: int, polygonSet) -> TRangePlan:
        ctx = _lib.context(device)
        ps = polygonSet if isinstance(polygonSet, PolygonSet) else PolygonSet(polygonSet)
        key = (ctx.device, ps.digest())
        h = self._plans.get(key)
        if h is None:
            p = TRangePlan(ctx, self.index, ps)
            h, p._owned = p.handle, False  # the cache owns it
            self._plans.put(key, h)
        view = TRangePlan.__new__(TRangePlan)  # a borrowed view: close() never destroys
        view.ctx, view.handle, view._owned = ctx, h, False
        return view

    def run(self, window: PointWindow, polygonSet, groups: "TrajectoryGroups" = None):
        qt = self.conf.getQueryType()
        if qt not in (QueryType.WindowBased, QueryType.RealTime):
            raise ValueError("Not yet support")
        plan = self.plan(window.x.device.index, polygonSet)
        if qt == QueryType.RealTime:
            return plan.points(window)
        g = groups if groups is not None else TrajectoryGroups(window)
        try:
            return g.trange(self.index, polygonSet, plan=plan)
        finally:
            if groups is None:
                g.close()

    def __del__(self):
        plans = getattr(self, "_plans", None)
        if plans is not None:
            plans.close()


class PointTFilterQuery:
    """tFilter/PointTFilterQuery.java windowBased: the trajectories whose objID is in trajIDSet (Strings or
    keys), each whole; an empty set = every trajectory (:92-95).  A String the window's dictionary never
    saw matches nothing."""

    def __init__(self, conf: QueryConfiguration, index: UniformGrid = None):
        self.conf = conf
        self.index = index

    def run(self, window: PointWindow, trajIDSet=(), groups: "TrajectoryGroups" = None) -> "SubTrajectories":
        if self.conf.getQueryType() != QueryType.WindowBased:
            raise ValueError("Not yet support")
        ids = _traj_id_keys(window, trajIDSet)
        if ids is not None and len(ids) == 0:  # a non-empty set none of whose Strings the window can hold
            e = np.empty(0)
            return SubTrajectories(window, e.astype(np.int64), np.zeros(1, np.int64), e, e.copy(), e.astype(np.int64),
                                   e.astype(np.uint32))
        g = groups if groups is not None else TrajectoryGroups(window)
        try:
            return g.tfilter(() if ids is None else ids)
        finally:
            if groups is None:
                g.close()


# ----------------------------------------------------------------------------------------
# tAggregate (the windowed heatmap: per grid cell, how long each objID stayed)
# ----------------------------------------------------------------------------------------
TAGG_KINDS = ("ALL", "SUM", "AVG", "MIN", "MAX")


def tagg_rows(aggregateFunction: str, table):
    """gf_tagg_rows (pure host): the emitted rows of one aggregate function from a per-cell table (the
    dict of TAggregateGroups.cells()) -> (kind, emit bool[cells], value int64[cells], key int64[cells])."""
    cols = {k: np.ascontiguousarray(table[k], np.int64) for k in
            ("count", "multi", "sum", "minLen", "minKey", "maxLen", "maxKey")}
    m = len(cols["count"])
    emit, value, key = np.zeros(m, np.uint8), np.zeros(m, np.int64), np.zeros(m, np.int64)
    kind = C.c_int32()
    st = _lib.lib().gf_tagg_rows(str(aggregateFunction).encode(), m, *(cols[k].ctypes.data for k in
                                 ("count", "multi", "sum", "minLen", "minKey", "maxLen", "maxKey")),
                                 emit.ctypes.data, value.ctypes.data, key.ctypes.data, C.byref(kind))
    _lib.check(st, None, "gf_tagg_rows")
    return TAGG_KINDS[kind.value], emit.astype(bool), value, key


class TAggregateGroups:
    """gf_tagg of one window: the window grouped by (cell, objID) on the device (stable; cells and,
    inside a cell, objIDs in first-occurrence order).  regroup(window, grid) reuses the device
    workspace for the next window; run() computes the statistics."""

    def __init__(self, window: PointWindow, grid: UniformGrid):
        self.handle = C.c_void_p()
        self.regroup(window, grid)

    def regroup(self, window: PointWindow, grid: UniformGrid):
        self.window = window
        self.ctx = _lib.context(window.x.device.index)
        pts = window.c_struct()
        _lib.check(_lib.lib().gf_tagg_group(self.ctx.handle, C.byref(grid.c_grid), C.byref(pts), C.byref(self.handle)),
                   self.ctx.handle, "gf_tagg_group")
        c, g, n = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().gf_tagg_info(self.handle, C.byref(c), C.byref(g), C.byref(n)), None, "gf_tagg_info")
        self.ncells, self.ngroups, self.n = c.value, g.value, n.value
        return self

    def set_thresholds(self, long_group: int = 0, big_cell: int = 0):
        """Testing / tuning: groups of at least `long_group` points and cells of at least `big_cell`
        objIDs take the block paths at the next run() (0: the defaults)."""
        _lib.check(_lib.lib().gf_tagg_set_thresholds(self.handle, int(long_group), int(big_cell)), None,
                   "gf_tagg_set_thresholds")

    def run(self):
        pts = self.window.c_struct()
        _lib.check(_lib.lib().gf_tagg_run(self.handle, C.byref(pts)), self.ctx.handle, "gf_tagg_run")
        return self

    def cells(self):
        """The per-cell table on the host: dict of cx, cy (int32) and count, multi, sum, minLen, minKey,
        maxLen, maxKey (int64), one entry per cell."""
        m = self.ncells
        t = {k: np.empty(m, np.int32) for k in ("cx", "cy")}
        t.update({k: np.empty(m, np.int64) for k in ("count", "multi", "sum", "minLen", "minKey", "maxLen", "maxKey")})
        got = C.c_int64()
        st = _lib.lib().gf_tagg_read_cells(self.handle, *(a.ctypes.data for a in t.values()), m, C.byref(got))
        _lib.check(st, self.ctx.handle, "gf_tagg_read_cells")
        return t

    def all_rows(self):
        """The ALL maps as CSR on the host: (off int64[cells + 1], keys int64[groups], len int64[groups])."""
        off = np.zeros(self.ncells + 1, np.int64)
        keys, ln = np.empty(self.ngroups, np.int64), np.empty(self.ngroups, np.int64)
        c, g = C.c_int64(), C.c_int64()
        st = _lib.lib().gf_tagg_read_all(self.handle, off.ctypes.data, keys.ctypes.data, ln.ctypes.data, self.ncells,
                                         self.ngroups, C.byref(c), C.byref(g))
        _lib.check(st, self.ctx.handle, "gf_tagg_read_all")
        return off, keys, ln

    def close(self):
        h = getattr(self, "handle", None)
        if h and _lib._lib is not None:
            _lib._lib.gf_tagg_destroy(h)
            self.handle = C.c_void_p()

    __del__ = close


@dataclass
class TAggregateResult:
    """The emitted rows of TimeWindowProcessFunction (TAggregateQuery.java:498-613) as arrays, one row
    per emitted cell, cells in the order of their first point in the window: (cx, cy), count, and the
    payload -- ALL: the cell's {objID: length} map as CSR (off, keys, lens; objIDs in the order of
    their first point in the cell); SUM / AVG: value; MIN / MAX: (key, value).  start / end are the
    window's, carried through."""

    window: PointWindow
    kind: str
    cx: np.ndarray
    cy: np.ndarray
    count: np.ndarray
    value: np.ndarray
    key: np.ndarray
    off: np.ndarray
    keys: np.ndarray
    lens: np.ndarray
    start: int = 0
    end: int = 0

    def __len__(self):
        return len(self.cx)

    def cell_ids(self):
        """The rows' cell-ID Strings ("%05d%05d", HelperClass.java:118-120)."""
        return [generateCellIDStr(a, b) for a, b in zip(self.cx.tolist(), self.cy.tolist())]

    def tuples(self):
        """Tuple5<cellID, count, winStart, winEnd, map>: objID Strings through the window's dictionary;
        SUM / AVG carry the reference's "" key."""
        ids = self.cell_ids()
        if self.kind == "ALL":
            names = self.window.objid_strings(self.keys) if len(self.keys) else []
            lens, off = self.lens.tolist(), self.off.tolist()
            maps = [OrderedDict(zip(names[off[j]:off[j + 1]], lens[off[j]:off[j + 1]])) for j in range(len(ids))]
        elif self.kind in ("SUM", "AVG"):
            maps = [{"": v} for v in self.value.tolist()]
        else:
            names = self.window.objid_strings(self.key) if len(self.key) else []
            maps = [{s: v} for s, v in zip(names, self.value.tolist())]
        return [(i, c, self.start, self.end, m) for i, c, m in zip(ids, self.count.tolist(), maps)]


class PointTAggregateQuery:
    """tAggregate/PointTAggregateQuery.java + TAggregateQuery.java:498-613 -- the windowed heatmap: per
    grid cell of the window, the objIDs seen there, how long each stayed (max ts - min ts of its points
    in the cell) and ALL / SUM / AVG / MIN / MAX of those stays (names as equalsIgnoreCase; any other
    name behaves as ALL).  WindowBased with the TIME window only: the RealTime variant reads the wall
    clock and COUNT windows are per-cell streams; both raise as unsupported."""

    def __init__(self, conf: QueryConfiguration, index: UniformGrid = None):
        self.conf = conf
        self.index = index

    def run(self, window: PointWindow, aggregateFunction: str, windowType: str = "TIME", groups=None) -> TAggregateResult:
        if self.conf.getQueryType() != QueryType.WindowBased or str(windowType).upper() == "COUNT":
            raise ValueError("Not yet support")
        if self.index is None:
            raise ValueError("PointTAggregateQuery needs the grid")
        g = groups.regroup(window, self.index) if groups is not None else TAggregateGroups(window, self.index)
        try:
            t = g.run().cells()
            kind, emit, value, key = tagg_rows(aggregateFunction, t)
            off = np.zeros(1, np.int64)
            keys = lens = np.empty(0, np.int64)
            if kind == "ALL":
                off, keys, lens = g.all_rows()
        finally:
            if groups is None:
                g.close()
        return TAggregateResult(window, kind, t["cx"][emit], t["cy"][emit], t["count"][emit], value[emit], key[emit],
                                off, keys, lens, window.start, window.end)


# ----------------------------------------------------------------------------------------
# tKnn (the window-based trajectory kNN)
# ----------------------------------------------------------------------------------------
@dataclass
class TKNNResult:
    """The rows of the window-based tKnn, nearest first: objID (keys), dist = D_t, cells = cells_t and
    the whole trajectory of row j as points [off[j], off[j + 1]) of x, y, ts, idx (idx = index in the
    window) in arrival order.  The contract is include/geoflink_hip.h's."""

    window: PointWindow
    objID: np.ndarray
    dist: np.ndarray
    cells: np.ndarray
    off: np.ndarray
    x: np.ndarray
    y: np.ndarray
    ts: np.ndarray
    idx: np.ndarray
    info: dict = None

    def __len__(self):
        return len(self.objID)

    def objid_strings(self):
        """The rows' objID Strings, through the window's dictionary."""
        return self.window.objid_strings(self.objID)

    def tuples(self):
        """(objID String, distance) per row."""
        return list(zip(self.objid_strings(), self.dist.tolist()))

    def linestrings(self, repeat: bool = False):
        """The rows' coordinate lists [(x, y), ...]; repeat=True: each list repeated cells times, the
        reference's LineString (its join emits the trajectory once per cell list holding it)."""
        off, xs, ys = self.off.tolist(), self.x.tolist(), self.y.tolist()
        out = []
        for j in range(len(off) - 1):
            ls = list(zip(xs[off[j]:off[j + 1]], ys[off[j]:off[j + 1]]))
            out.append(ls * int(self.cells[j]) if repeat else ls)
        return out


class PointPointTKNNQuery:
    """tKnn/PointPointTKNNQuery.java windowBased (run) and windowBasedNaive (runNaive) +
    TKNNQuery.kNNEvaluationWindowed: the k trajectories nearest to a query point, each whole.  The
    window mode never compares a distance with the radius (a quirk kept): the radius only selects the
    cells.  WindowBased only; the RealTime and CountBased variants raise as unsupported."""

    def __init__(self, conf: QueryConfiguration, index: UniformGrid = None):
        self.conf = conf
        self.index = index

    def _run(self, window, queryPoint, queryRadius, k, naive, groups):
        if self.conf.getQueryType() != QueryType.WindowBased:
            raise ValueError("Not yet support")
        if self.index is None:
            raise ValueError("PointPointTKNNQuery needs the grid")
        g = groups if groups is not None else TrajectoryGroups(window)
        try:
            return g.tknn(self.index, queryPoint, queryRadius, k, naive=naive)
        finally:
            if groups is None:
                g.close()

    def run(self, window: PointWindow, queryPoint: Point, queryRadius: float, k: int, groups=None) -> TKNNResult:
        """groups: the window's TrajectoryGroups, if the caller has grouped it already."""
        return self._run(window, queryPoint, queryRadius, k, False, groups)

    def runNaive(self, window: PointWindow, queryPoint: Point, queryRadius: float, k: int, groups=None) -> TKNNResult:
        return self._run(window, queryPoint, queryRadius, k, True, groups)


# ----------------------------------------------------------------------------------------
# tJoin (the window-based trajectory join)
# ----------------------------------------------------------------------------------------
@dataclass
class TJoinResult:
    """The rows of the window-based tJoin, ascending by (ordinary rank, query rank): per row the two
    objID keys, p_first / q_latest (window indices of the first matching ordinary point and the latest
    matching query point), emit (both trajectories have >= 2 points) and oslot / qslot, the row's
    trajectories in `ordinary` / `query` (SubTrajectories: each emitted trajectory whole and once; -1 where
    emit is False).  The contract is include/geoflink_hip.h's."""

    okey: np.ndarray
    qkey: np.ndarray
    p_first: np.ndarray
    q_latest: np.ndarray
    emit: np.ndarray
    oslot: np.ndarray
    qslot: np.ndarray
    ordinary: SubTrajectories
    query: SubTrajectories
    info: dict = None

    def __len__(self):
        return len(self.okey)

    @property
    def first_point(self):
        """The reference's firstPoint per ordinary objID: {objID key: the minimum of p_first over its rows}."""
        out = {}
        for k, p in zip(self.okey.tolist(), self.p_first.tolist()):
            out[k] = min(out.get(k, p), p)
        return out

    def point_pairs(self):
        """runSingle's / the join stage's Tuple2<Point, Point> per row as window indices: (firstPoint of the
        row's ordinary objID, q_latest)."""
        fp = self.first_point
        return [(fp[k], q) for k, q in zip(self.okey.tolist(), self.q_latest.tolist())]

    def trajectory_pairs(self):
        """The emitted rows as (ordinary slot, query slot): Tuple2<LineString, LineString>."""
        return list(zip(self.oslot[self.emit].tolist(), self.qslot[self.emit].tolist()))


class PointPointTJoinQuery:
    """tJoin/PointPointTJoinQuery.java windowBased (run) and commonSingle (runSingle) + TJoinQuery.java: the
    pairs of trajectories with a point of one within joinDistance of a point of the other, each pair once,
    each trajectory whole.  WindowBased only; the RealTime variants raise as unsupported."""

    def __init__(self, conf: QueryConfiguration, index: UniformGrid = None):
        self.conf = conf
        self.index = index

    def _check(self):
        _require_supported(self.conf)
        if self.conf.getQueryType() != QueryType.WindowBased:
            raise ValueError("Not yet support")
        if self.index is None:
            raise ValueError("PointPointTJoinQuery needs the grid")

    def run(self, ordinaryWindow: PointWindow, queryWindow: PointWindow, joinDistance: float, groups=None) -> TJoinResult:
        """groups: (ordinary TrajectoryGroups, query TrajectoryGroups), if the caller has grouped the windows already."""
        self._check()
        go, gq = groups if groups is not None else (TrajectoryGroups(ordinaryWindow), TrajectoryGroups(queryWindow))
        try:
            return go.tjoin(gq, self.index, joinDistance)
        finally:
            if groups is None:
                go.close()
                gq.close()

    def runSingle(self, window: PointWindow, joinDistance: float, groups=None) -> TJoinResult:
        self._check()
        g = groups if groups is not None else TrajectoryGroups(window)
        try:
            return g.tjoin(g, self.index, joinDistance, single=True)
        finally:
            if groups is None:
                g.close()


# ----------------------------------------------------------------------------------------
# polygon / linestring windows against query points
# ----------------------------------------------------------------------------------------
class GeometryIndex:
    """gf_geom_prepare of one GeometryWindow on one grid: per-object envelopes, cell rectangles,
    validity and vertex counts, reusable by many queries (the window's tensors are borrowed and kept
    alive here)."""

    def __init__(self, window: GeometryWindow, grid: UniformGrid):
        self.ctx = _lib.context(window.vert_off.device.index)
        self.handle = C.c_void_p()
        self.prepare(window, grid)

    def prepare(self, window: GeometryWindow, grid: UniformGrid = None):
        """Async: this index for `window` (the next window of a continuous query): the threshold stays, the
        device arrays are reused and only grow, so a window no larger than an earlier one allocates nothing
        and does not wait."""
        grid = grid or self.grid
        g = window.c_struct()
        _lib.check(_lib.lib().gf_geom_prepare(self.ctx.handle, C.byref(grid.c_grid), C.byref(g), C.byref(self.handle)),
                   self.ctx.handle, "gf_geom_prepare")
        self.window, self.grid = window, grid

    def info(self) -> dict:
        v = [C.c_int64() for _ in range(4)]
        _lib.check(_lib.lib().gf_geom_index_info(self.handle, *(C.byref(c) for c in v)), self.ctx.handle, "gf_geom_index_info")
        return dict(zip(("nobj", "nvert", "invalid", "wide"), (c.value for c in v)))

    def read(self):
        """(env [nobj, 4] = x1, y1, x2, y2; cells [nobj, 4] = cx1, cy1, cx2, cy2) as numpy arrays"""
        n = self.window.nobj
        env, cells = np.zeros((n, 4), np.float64), np.zeros((n, 4), np.int32)
        _lib.check(_lib.lib().gf_geom_index_read(self.handle, env.ctypes.data, cells.ctypes.data), self.ctx.handle,
                   "gf_geom_index_read")
        return env, cells

    def set_thresholds(self, wide_vertices: int = 0):
        _lib.check(_lib.lib().gf_geom_index_set_thresholds(self.handle, int(wide_vertices)), self.ctx.handle,
                   "gf_geom_index_set_thresholds")

    def close(self):
        h = getattr(self, "handle", None)
        if h and _lib._lib is not None:
            _lib._lib.gf_geom_index_destroy(h)
        self.handle = None

    def __del__(self):
        self.close()


class _GeomWindowQuery(SpatialOperator):
    """What the four geometry-window operators share: the cached gf_geom_query of a point set and the
    index of the window (prepared here unless the caller shares one)."""

    _destroy_name = "gf_geom_query_destroy"
    _kind = _lib.GEOM_POLYGON

    def query(self, device: int, queryPoints, queryRadius: float):
        """(context, gf_geom_query) of this point set on `device` (cached by query contents)."""
        _require_supported(self.conf)
        qs = list(queryPoints)
        qx = np.array([q.x for q in qs], np.float64)
        qy = np.array([q.y for q in qs], np.float64)
        ctx = _lib.context(device)
        key = (ctx.device, tuple(qx.tolist()), tuple(qy.tolist()), float(queryRadius),
               bool(self.conf.approximateQuery), int(self.conf.distanceMetric))
        q = self._plans.get(key)
        if q is None:
            q = C.c_void_p()
            st = _lib.lib().gf_geom_query_create(ctx.handle, C.byref(self.index.c_grid), qx.ctypes.data, qy.ctypes.data,
                                                 len(qs), float(queryRadius), int(self.conf.approximateQuery),
                                                 int(self.conf.distanceMetric), C.byref(q))
            _lib.check(st, ctx.handle, "gf_geom_query_create")
            self._plans.put(key, q)
        self._last = (ctx, q)
        return ctx, q

    def _index(self, window: GeometryWindow, index):
        if window.kind != self._kind:
            raise ValueError(f"{type(self).__name__}: the window holds the other kind of geometry")
        if index is None:
            return GeometryIndex(window, self.index)
        if index.window is not window:
            raise ValueError("the index was prepared for another window")
        return index

    def info(self) -> dict:
        """gf_geom_info of the last run: filtered, all_guaranteed, tested, wave_path"""
        ctx, q = self._last
        v = [C.c_int64() for _ in range(4)]
        _lib.check(_lib.lib().gf_geom_info(q, *(C.byref(c) for c in v)), ctx.handle, "gf_geom_info")
        return dict(zip(("filtered", "all_guaranteed", "tested", "wave_path"), (c.value for c in v)))

    def __del__(self):
        plans = getattr(self, "_plans", None)
        if plans is not None:
            plans.close()


class PolygonPointRangeQuery(_GeomWindowQuery):
    """range/PolygonPointRangeQuery.java -- a window of polygons against a set of query points."""

    def run(self, window: GeometryWindow, queryPointSet, queryRadius: float, index: GeometryIndex = None) -> RangeResult:
        import torch

        ix = self._index(window, index)
        ctx, q = self.query(window.vert_off.device.index, queryPointSet, queryRadius)
        dev = window.vert_off.device
        bitmap = torch.zeros(max(1, (window.nobj + 63) // 64), dtype=torch.int64, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().gf_geom_range_run(q, ix.handle, bitmap.data_ptr(), counts.data_ptr()), ctx.handle,
                   "gf_geom_range_run")
        res = RangeResult(window, bitmap, counts, None, 1, ctx)
        if index is None:
            ctx.synchronize()  # the index made here goes with this call
            ix.close()
        return res


class LineStringPointRangeQuery(PolygonPointRangeQuery):
    """range/LineStringPointRangeQuery.java -- a window of linestrings against a set of query points."""

    _kind = _lib.GEOM_LINESTRING


class PolygonPointKNNQuery(_GeomWindowQuery):
    """knn/PolygonPointKNNQuery.java -- the k polygons of a window nearest to one query point within r."""

    def enqueue(self, window: GeometryWindow, queryPoint: Point, queryRadius: float, k: int, record, index: GeometryIndex):
        """Async: the window's record into `record` (a torch uint8 device tensor of knn_record_bytes(k) or
        an address); `index` must outlive the record's completion."""
        ix = self._index(window, index)
        ctx, q = self.query(window.vert_off.device.index, [queryPoint], queryRadius)
        addr = record if isinstance(record, int) else record.data_ptr()
        _lib.check(_lib.lib().gf_geom_knn_enqueue(q, ix.handle, int(k), C.c_void_p(addr)), ctx.handle, "gf_geom_knn_enqueue")
        return ctx

    def run(self, window: GeometryWindow, queryPoint: Point, queryRadius: float, k: int, index: GeometryIndex = None) -> KNNResult:
        import torch

        if k is None or int(k) < 1:
            raise ValueError("k must be >= 1 (PriorityQueue initialCapacity < 1)")
        ix = self._index(window, index)
        rec = torch.zeros(knn_record_bytes(k), dtype=torch.uint8, device=window.vert_off.device)
        self.enqueue(window, queryPoint, queryRadius, k, rec, ix)
        raw = rec.cpu().numpy().tobytes()  # (waits for the stream)
        if index is None:
            ix.close()
        st, o, d, i = decode_knn_record(raw, int(k))
        assert st == 0, "a geometry-window record is always final"
        return KNNResult(window.start, window.end, o, d, i)


class LineStringPointKNNQuery(PolygonPointKNNQuery):
    """knn/LineStringPointKNNQuery.java -- the k linestrings of a window nearest to one query point within r."""

    _kind = _lib.GEOM_LINESTRING


# ----------------------------------------------------------------------------------------
# polygon / linestring windows against polygon / linestring queries
# ----------------------------------------------------------------------------------------
class _GeomPairQuery(_GeomWindowQuery):
    """The query side of the eight geometry-pair operators: a gf_geom_query built from a PolygonSet or a
    LineStringSet (or the Polygon / LineString objects that make one), cached by the set's contents.
    chain_mode = 1 builds the query without run-envelope pruning (tests, tools/bench_geompair.py)."""

    _query_kind = _lib.GEOM_POLYGON
    chain_mode = 0

    def _query_set(self, queries):
        if isinstance(queries, list) and len(queries) == 1 and isinstance(queries[0], (PolygonSet, LineStringSet)):
            queries = queries[0]  # the kNN operators wrap their one query in a list
        if self._query_kind == _lib.GEOM_POLYGON:
            if isinstance(queries, Polygon):
                queries = [queries]
            return queries if isinstance(queries, PolygonSet) else PolygonSet(queries)
        if isinstance(queries, LineString):
            queries = [queries]
        return queries if isinstance(queries, LineStringSet) else LineStringSet(queries)

    def query(self, device: int, queries, queryRadius: float):
        # WindowBased only: the reference's RealTime bodies of these operators differ from their window bodies
        if self.conf.getQueryType() is not QueryType.WindowBased:
            raise ValueError("Not yet support")
        qset = self._query_set(queries)
        ctx = _lib.context(device)
        key = (ctx.device, self._query_kind, qset.digest(), float(queryRadius), bool(self.conf.approximateQuery),
               int(self.conf.distanceMetric), int(self.chain_mode))
        q = self._plans.get(key)
        if q is None:
            q = C.c_void_p()
            polygons = self._query_kind == _lib.GEOM_POLYGON
            name = "gf_geom_query_create_polygons" if polygons else "gf_geom_query_create_linestrings"
            cs = qset.c_struct()
            st = getattr(_lib.lib(), name)(ctx.handle, C.byref(self.index.c_grid), C.byref(cs), float(queryRadius),
                                           int(self.conf.approximateQuery), int(self.conf.distanceMetric), C.byref(q))
            _lib.check(st, ctx.handle, name)
            if self.chain_mode:
                _lib.check(_lib.lib().gf_geom_query_set_chain_mode(q, int(self.chain_mode)), ctx.handle,
                           "gf_geom_query_set_chain_mode")
            self._plans.put(key, q)
        self._last = (ctx, q)
        return ctx, q


class PolygonPolygonRangeQuery(_GeomPairQuery, PolygonPointRangeQuery):
    """range/PolygonPolygonRangeQuery.java -- a window of polygons against a set of query polygons."""


class PolygonLineStringRangeQuery(_GeomPairQuery, PolygonPointRangeQuery):
    """range/PolygonLineStringRangeQuery.java -- a window of polygons against a set of query linestrings."""

    _query_kind = _lib.GEOM_LINESTRING


class LineStringPolygonRangeQuery(_GeomPairQuery, LineStringPointRangeQuery):
    """range/LineStringPolygonRangeQuery.java -- a window of linestrings against a set of query polygons."""


class LineStringLineStringRangeQuery(_GeomPairQuery, LineStringPointRangeQuery):
    """range/LineStringLineStringRangeQuery.java -- a window of linestrings against a set of query linestrings."""

    _query_kind = _lib.GEOM_LINESTRING


class PolygonPolygonKNNQuery(_GeomPairQuery, PolygonPointKNNQuery):
    """knn/PolygonPolygonKNNQuery.java -- the k polygons of a window nearest to one query polygon within r."""


class PolygonLineStringKNNQuery(_GeomPairQuery, PolygonPointKNNQuery):
    """knn/PolygonLineStringKNNQuery.java -- the k polygons of a window nearest to one query linestring within r."""

    _query_kind = _lib.GEOM_LINESTRING


class LineStringPolygonKNNQuery(_GeomPairQuery, LineStringPointKNNQuery):
    """knn/LineStringPolygonKNNQuery.java -- the k linestrings of a window nearest to one query polygon within r."""


class LineStringLineStringKNNQuery(_GeomPairQuery, LineStringPointKNNQuery):
    """knn/LineStringLineStringKNNQuery.java -- the k linestrings of a window nearest to one query linestring
    within r."""

    _query_kind = _lib.GEOM_LINESTRING


# ----------------------------------------------------------------------------------------
# geometry-stream joins: a polygon / linestring window joined with a second stream
# ----------------------------------------------------------------------------------------
@dataclass
class GeomJoinResult:
    """The distinct pairs of one join window, sorted by (ordinary index, query index), each with its
    multiplicity m = the number of cell keys the pair shares (min(m, 2^32 - 1)): Flink's equi-join emits
    the pair once per shared key."""
    pairs: np.ndarray         # int64 [n, 2]
    multiplicity: np.ndarray  # int64 [n]
    nrep: int                 # the sum of the multiplicities, as the device counted it

    def replicated(self) -> np.ndarray:
        """the reference's output multiset: every pair repeated m times, int64 [nrep, 2]"""
        return np.repeat(self.pairs, self.multiplicity, axis=0)


class _GeomJoinQuery(SpatialOperator):
    """What the six geometry-stream joins share (gf_geom_join_run / gf_geom_join_run_points): the ordinary
    window's index on uGrid, the query side on qGrid, one joiner per device reused across windows.
    RealTime calls windowBased with slide = size in the reference, so both query types run the same window
    evaluation.  tile_side / long_tiles / brute are gf_geom_join_set_tuning's (tests, tools); results never
    depend on them."""

    _kind = _lib.GEOM_POLYGON
    _query_kind = 0          # 0: a point window
    _first_is_ordinary = 0   # PolygonLineStringJoinQuery: getDistance(polygon, lineString)
    tile_side = 0
    long_tiles = 0
    brute = 0

    def __init__(self, conf: QueryConfiguration, uGrid: UniformGrid, qGrid: UniformGrid = None):
        super().__init__(conf, uGrid)
        self.index2 = qGrid if qGrid is not None else uGrid
        self._joiners = {}
        self._last = None

    def _joiner(self, ctx):
        j = self._joiners.get(ctx.device)
        if j is None:
            j = C.c_void_p()
            _lib.check(_lib.lib().gf_geom_join_create(ctx.handle, C.byref(j)), ctx.handle, "gf_geom_join_create")
            self._joiners[ctx.device] = j
        return j

    @staticmethod
    def _side(name, window, index, kind, grid):
        """(index, made here) of a geometry side, checked as _GeomWindowQuery._index checks its window"""
        if not isinstance(window, GeometryWindow) or window.kind != kind:
            raise ValueError(f"{name}: the window holds the other kind of geometry")
        if index is None:
            return GeometryIndex(window, grid), True
        if index.window is not window:
            raise ValueError("the index was prepared for another window")
        return index, False

    def run(self, ordinaryWindow, queryWindow, queryRadius: float, index: GeometryIndex = None,
            query_index: GeometryIndex = None) -> GeomJoinResult:
        import torch

        _require_supported(self.conf)
        name = type(self).__name__
        if self._query_kind == 0 and not isinstance(queryWindow, PointWindow):
            raise ValueError(f"{name}: the query window must be a PointWindow")
        ix, own = self._side(name, ordinaryWindow, index, self._kind, self.index)
        qix, qown = (None, False) if self._query_kind == 0 else self._side(name, queryWindow, query_index, self._query_kind,
                                                                           self.index2)
        dev = ordinaryWindow.vert_off.device
        ctx = _lib.context(dev.index)
        L = _lib.lib()
        j = self._joiner(ctx)
        _lib.check(L.gf_geom_join_set_tuning(j, int(self.tile_side), int(self.long_tiles), int(self.brute)), ctx.handle,
                   "gf_geom_join_set_tuning")
        self._last = (ctx, j)
        approx, metric = int(self.conf.approximateQuery), int(self.conf.distanceMetric)
        pts = queryWindow.c_struct() if qix is None else None
        cap = max(1024, 2 * (ordinaryWindow.n + queryWindow.n))
        try:
            for _ in range(2):
                pairs = torch.empty(3 * cap, dtype=torch.int32, device=dev)
                npairs, nrep = C.c_int64(), C.c_int64()
                if qix is None:
                    what = "gf_geom_join_run_points"
                    st = L.gf_geom_join_run_points(j, ix.handle, C.byref(self.index2.c_grid), C.byref(pts), float(queryRadius),
                                                   approx, metric, pairs.data_ptr(), cap, C.byref(npairs), C.byref(nrep))
                else:
                    what = "gf_geom_join_run"
                    st = L.gf_geom_join_run(j, ix.handle, qix.handle, float(queryRadius), approx, metric,
                                            int(self._first_is_ordinary), pairs.data_ptr(), cap, C.byref(npairs), C.byref(nrep))
                if st == _lib.GF_ERR_CAPACITY:
                    cap = int(npairs.value)
                    continue
                _lib.check(st, ctx.handle, what)
                m = int(npairs.value)
                out = pairs[: 3 * m].cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 3)
                out = out[np.lexsort((out[:, 1], out[:, 0]))]
                return GeomJoinResult(np.ascontiguousarray(out[:, :2]), np.ascontiguousarray(out[:, 2]), int(nrep.value))
            raise _lib.GeoFlinkError(_lib.GF_ERR_CAPACITY, "join output kept growing")
        finally:
            if own:
                ix.close()  # (the run calls are synchronous: nothing in flight reads the index)
            if qown:
                qix.close()

    def info(self) -> dict:
        """gf_geom_join_info of the last run"""
        ctx, j = self._last
        v = [C.c_int64() for _ in range(6)]
        _lib.check(_lib.lib().gf_geom_join_info(j, *(C.byref(c) for c in v)), ctx.handle, "gf_geom_join_info")
        return dict(zip(("candidates", "box_dropped", "tested", "wave_path", "long_objects", "long_queries"),
                        (c.value for c in v)))

    def close(self):
        joiners, self._joiners = getattr(self, "_joiners", {}), {}
        for j in joiners.values():
            if _lib._lib is not None:
                _lib._lib.gf_geom_join_destroy(j)

    def __del__(self):
        self.close()


class PolygonPointJoinQuery(_GeomJoinQuery):
    """join/PolygonPointJoinQuery.java -- a polygon stream joined with a point stream."""


class LineStringPointJoinQuery(_GeomJoinQuery):
    """join/LineStringPointJoinQuery.java -- a linestring stream joined with a point stream."""

    _kind = _lib.GEOM_LINESTRING


class PolygonPolygonJoinQuery(_GeomJoinQuery):
    """join/PolygonPolygonJoinQuery.java -- a polygon stream joined with a polygon stream."""

    _query_kind = _lib.GEOM_POLYGON


class PolygonLineStringJoinQuery(_GeomJoinQuery):
    """join/PolygonLineStringJoinQuery.java -- a polygon stream joined with a linestring stream; the distance
    takes the ORDINARY polygon first (getDistance(poly, q)), unlike the other five."""

    _query_kind = _lib.GEOM_LINESTRING
    _first_is_ordinary = 1


class LineStringPolygonJoinQuery(_GeomJoinQuery):
    """join/LineStringPolygonJoinQuery.java -- a linestring stream joined with a polygon stream."""

    _kind = _lib.GEOM_LINESTRING
    _query_kind = _lib.GEOM_POLYGON


class LineStringLineStringJoinQuery(_GeomJoinQuery):
    """join/LineStringLineStringJoinQuery.java -- a linestring stream joined with a linestring stream."""

    _kind = _lib.GEOM_LINESTRING
    _query_kind = _lib.GEOM_LINESTRING


__all__ = [
    "PolygonPointJoinQuery", "LineStringPointJoinQuery", "PolygonPolygonJoinQuery", "PolygonLineStringJoinQuery",
    "LineStringPolygonJoinQuery", "LineStringLineStringJoinQuery", "GeomJoinResult",
    "PolygonPolygonRangeQuery", "PolygonLineStringRangeQuery", "LineStringPolygonRangeQuery", "LineStringLineStringRangeQuery",
    "PolygonPolygonKNNQuery", "PolygonLineStringKNNQuery", "LineStringPolygonKNNQuery", "LineStringLineStringKNNQuery",
    "GeometryIndex", "PolygonPointRangeQuery", "LineStringPointRangeQuery", "PolygonPointKNNQuery", "LineStringPointKNNQuery",
    "LineString", "LineStringSet", "PointLineStringRangeQuery", "PointLineStringKNNQuery", "PointLineStringJoinQuery",
    "PointPointTJoinQuery", "TJoinResult",
    "PointPolygonTRangeQuery", "PointTFilterQuery", "TRangePlan",
    "PointPointTKNNQuery", "TKNNResult",
    "PointTAggregateQuery", "TAggregateResult", "TAggregateGroups", "tagg_rows",
    "PointTStatsQuery", "TStatsResult", "SubTrajectories", "TrajectoryGroups", "group_by_objid", "sub_trajectories",
    "synthetic_clustered", "QueryType", "QueryConfiguration", "PointPointRangeQuery", "PointPolygonRangeQuery", "PointPointKNNQuery",
    "PointPointJoinQuery", "PointPolygonJoinQuery", "RangeResult", "KNNResult", "knn_merge_host", "assign_cells", "bucket_by_cell",
    "synthetic_uniform", "Point", "Polygon", "PointWindow", "knn_record_bytes", "decode_knn_record",
]
