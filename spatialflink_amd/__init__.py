"""spatialflink_amd -- MI355X-native window-evaluation hot path of GeoFlink / SpatialFlink.

The Java operators' per-window bodies (range, kNN, join) run as hand-written HIP kernels
for gfx950 behind the C ABI in include/geoflink_hip.h; this package is the host-side
mirror of the reference operator API (UniformGrid, Point, Polygon, QueryConfiguration,
PointPointRangeQuery, PointPolygonRangeQuery, PointPointKNNQuery, PointPointJoinQuery,
PointPolygonKNNQuery, PointPolygonJoinQuery, PointTStatsQuery, PointTAggregateQuery,
PointPointTKNNQuery, PointPointTJoinQuery, LineString and the PointLineString{Range,KNN,Join}Query
operators, the PolygonPoint / LineStringPoint {Range,KNN}Query operators over geometry windows, and the
{Polygon,LineString}{Polygon,LineString}{Range,KNN}Query operators: geometry windows against geometry queries;
{Polygon,LineString}{Point,Polygon,LineString}JoinQuery: geometry windows joined with a second stream).
"""
from . import _lib, sharding
from .spatialIndices import UniformGrid, generateCellIDStr, getIntCellIndices, padLeadingZeroesToInt
from .spatialObjects import (GeometryWindow, LineString, LineStringSet, LineStringWindow, ObjIdDict, Point, PointWindow,
                             Polygon, PolygonSet, PolygonWindow)
from .spatialOperators import (KNNResult, PinnedRecords, PointPointJoinQuery, PointPointKNNQuery, PointPointRangeQuery,
                               PointPolygonJoinQuery, PointPolygonKNNQuery, PointTStatsQuery, SubTrajectories,
                               TrajectoryGroups, TStatsResult, group_by_objid, sub_trajectories,
                               PointTAggregateQuery, TAggregateGroups, TAggregateResult, tagg_rows,
                               PointPointTKNNQuery, TKNNResult, PointPointTJoinQuery, TJoinResult,
                               PointPolygonTRangeQuery, PointTFilterQuery, TRangePlan,
                               GeometryIndex, LineStringPointKNNQuery, LineStringPointRangeQuery, PolygonPointKNNQuery,
                               PolygonPointRangeQuery,
                               PolygonPolygonRangeQuery, PolygonLineStringRangeQuery, LineStringPolygonRangeQuery,
                               LineStringLineStringRangeQuery, PolygonPolygonKNNQuery, PolygonLineStringKNNQuery,
                               LineStringPolygonKNNQuery, LineStringLineStringKNNQuery,
                               PolygonPointJoinQuery, LineStringPointJoinQuery, PolygonPolygonJoinQuery,
                               PolygonLineStringJoinQuery, LineStringPolygonJoinQuery, LineStringLineStringJoinQuery,
                               GeomJoinResult,
                               PointLineStringJoinQuery, PointLineStringKNNQuery, PointLineStringRangeQuery,
                               PointPolygonRangeQuery, QueryConfiguration, QueryType, RangeResult, assign_cells,
                               bucket_by_cell, knn_merge_host, synthetic_uniform,
                               synthetic_clustered)
from .spatialStreams import Deserialization
from .windows import SlidingKNNQuery, SlidingRangeQuery, SlidingWindows

__all__ = [
    "PolygonPointJoinQuery", "LineStringPointJoinQuery", "PolygonPolygonJoinQuery", "PolygonLineStringJoinQuery",
    "LineStringPolygonJoinQuery", "LineStringLineStringJoinQuery", "GeomJoinResult",
    "PolygonPolygonRangeQuery", "PolygonLineStringRangeQuery", "LineStringPolygonRangeQuery", "LineStringLineStringRangeQuery",
    "PolygonPolygonKNNQuery", "PolygonLineStringKNNQuery", "LineStringPolygonKNNQuery", "LineStringLineStringKNNQuery",
    "GeometryWindow", "PolygonWindow", "LineStringWindow", "GeometryIndex", "PolygonPointRangeQuery",
    "LineStringPointRangeQuery", "PolygonPointKNNQuery", "LineStringPointKNNQuery",
    "LineString", "LineStringSet", "PointLineStringRangeQuery", "PointLineStringKNNQuery", "PointLineStringJoinQuery",
    "PointPointTJoinQuery", "TJoinResult",
    "PointPolygonTRangeQuery", "PointTFilterQuery", "TRangePlan",
    "PointPointTKNNQuery", "TKNNResult",
    "PointTAggregateQuery", "TAggregateResult", "TAggregateGroups", "tagg_rows",
    "PointTStatsQuery", "TStatsResult", "SubTrajectories", "TrajectoryGroups", "group_by_objid", "sub_trajectories",
    "SlidingWindows", "SlidingKNNQuery", "SlidingRangeQuery", "Deserialization", "PointPolygonKNNQuery", "PointPolygonJoinQuery",
    "UniformGrid", "ObjIdDict", "Point", "Polygon", "PolygonSet", "PointWindow", "QueryType", "QueryConfiguration",
    "PointPointRangeQuery", "PointPolygonRangeQuery", "PointPointKNNQuery", "PointPointJoinQuery", "RangeResult",
    "KNNResult", "PinnedRecords", "knn_merge_host", "assign_cells", "bucket_by_cell", "synthetic_uniform", "synthetic_clustered", "generateCellIDStr",
    "getIntCellIndices", "padLeadingZeroesToInt",
]
