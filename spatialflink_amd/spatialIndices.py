"""UniformGrid -- mirror of GeoFlink.spatialIndices.UniformGrid (UniformGrid.java).

Host-side grid arithmetic goes through the C ABI (gf_grid_make / gf_grid_layers /
gf_cell_of / gf_format_cell_id / gf_parse_cell_id) so the cell of a point is computed by
exactly the code the GPU kernels share (spatialflink_amd/csrc/gf_numerics.hpp).
The string cell-set helpers mirror the reference's HashSet<String> API for callers that
use it directly; the window evaluation itself never materialises these sets.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _lib

CELLINDEXSTRLENGTH = 5  # UniformGrid.java:40


def padLeadingZeroesToInt(cellIndex: int, desiredStringLength: int = CELLINDEXSTRLENGTH) -> str:
    """HelperClass.padLeadingZeroesToInt -- HelperClass.java:54-57"""
    return ("%0" + str(desiredStringLength) + "d") % cellIndex


def generateCellIDStr(x: int, y: int) -> str:
    """HelperClass.generateCellIDStr -- HelperClass.java:118-120"""
    buf = C.create_string_buffer(64)
    _lib.check(_lib.lib().gf_format_cell_id(int(x), int(y), buf, 64), None, "gf_format_cell_id")
    return buf.value.decode()


def getIntCellIndices(cellID: str):
    """HelperClass.getIntCellIndices -- HelperClass.java:263-276"""
    a, b = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().gf_parse_cell_id(cellID.encode(), C.byref(a), C.byref(b)), None, "gf_parse_cell_id")
    return [a.value, b.value]


class UniformGrid:
    """UniformGrid(int uniformGridRows, minX, maxX, minY, maxY) -- UniformGrid.java:74-85.

    cellLength = (maxX - minX) / n; the bounds are NOT squared (only the cellLength
    constructor squares them, see fromCellLength)."""

    def __init__(self, uniformGridRows: int, minX: float, maxX: float, minY: float, maxY: float):
        self._g = _lib.GfGrid()
        st = _lib.lib().gf_grid_make(int(uniformGridRows), float(minX), float(maxX), float(minY), float(maxY),
                                     C.byref(self._g))
        _lib.check(st, None, "UniformGrid: invalid bounds or partitions")

    @classmethod
    def fromCellLength(cls, cellLength: float, minX: float, maxX: float, minY: float, maxY: float):
        """UniformGrid(double cellLength, ...) -- UniformGrid.java:47-72 (+ adjustCoordinatesForSquareGrid
        :114-134): square the bounds, n = ceil(gridLength / cellLength), then the actual cell length."""
        xd, yd = maxX - minX, maxY - minY
        if xd > yd:
            diff = xd - yd
            maxY += diff / 2
            minY -= diff / 2
        elif yd > xd:
            diff = yd - xd
            maxX += diff / 2
            minX -= diff / 2
        gridLength = math.sqrt((minY - minY) ** 2 + (maxX - minX) ** 2)
        rows = gridLength / cellLength
        n = 1 if rows < 1 else int(math.ceil(rows))
        self = cls(n, minX, maxX, minY, maxY)
        return self

    # -- getters (UniformGrid.java:136-147)
    def getMinX(self): return self._g.minX
    def getMinY(self): return self._g.minY
    def getMaxX(self): return self._g.maxX
    def getMaxY(self): return self._g.maxY
    def getCellIndexStrLength(self): return CELLINDEXSTRLENGTH
    def getNumGridPartitions(self): return self._g.n
    def getCellLength(self): return self._g.cellLength

    @property
    def c_grid(self) -> _lib.GfGrid:
        return self._g

    def validKey(self, x: int, y: int) -> bool:
        """UniformGrid.java:224-229"""
        n = self._g.n
        return 0 <= x < n and 0 <= y < n

    def getGuaranteedNeighboringLayers(self, queryRadius: float) -> int:
        g, c = C.c_int32(), C.c_int32()
        _lib.lib().gf_grid_layers(C.byref(self._g), float(queryRadius), C.byref(g), C.byref(c))
        return g.value

    def getCandidateNeighboringLayers(self, queryRadius: float) -> int:
        g, c = C.c_int32(), C.c_int32()
        _lib.lib().gf_grid_layers(C.byref(self._g), float(queryRadius), C.byref(g), C.byref(c))
        return c.value

    def cellOf(self, x: float, y: float):
        a, b = C.c_int32(), C.c_int32()
        _lib.lib().gf_cell_of(C.byref(self._g), float(x), float(y), C.byref(a), C.byref(b))
        return a.value, b.value

    def assignGridCellID(self, x: float, y: float) -> str:
        """HelperClass.assignGridCellID(Coordinate, UniformGrid) -- HelperClass.java:104-116"""
        return generateCellIDStr(*self.cellOf(x, y))

    def getGirdCellsSet(self):
        n = self._g.n
        return {generateCellIDStr(i, j) for i in range(n) for j in range(n)}

    # -- neighbour-cell sets (UniformGrid.java:165-206, 261-293, 368-411)
    def _cells_of(self, query):
        # a Polygon or a LineString carries the cells under its bbox (UniformGrid.java:193-222, 399-426: the
        # polygon and linestring forms are the same per-bbox-cell unions), a Point or a cell id one cell
        gridIDsSet = getattr(query, "gridIDsSet", None)
        if gridIDsSet is not None:
            return list(gridIDsSet)
        return [query if isinstance(query, str) else query.gridID]

    def getGuaranteedNeighboringCells(self, queryRadius: float, query) -> set:
        out = set()
        gl = self.getGuaranteedNeighboringLayers(queryRadius)
        n = self._g.n
        for cellID in self._cells_of(query):
            if gl == 0:
                out.add(cellID)
            elif gl > 0:
                qx, qy = getIntCellIndices(cellID)
                for i in range(max(qx - gl, 0), min(qx + gl, n - 1) + 1):
                    for j in range(max(qy - gl, 0), min(qy + gl, n - 1) + 1):
                        out.add(generateCellIDStr(i, j))
        return out

    def getCandidateNeighboringCells(self, queryRadius: float, query, guaranteedNeighboringCellsSet) -> set:
        out = set()
        cl = self.getCandidateNeighboringLayers(queryRadius)
        n = self._g.n
        if cl <= 0:
            return out
        for cellID in self._cells_of(query):
            qx, qy = getIntCellIndices(cellID)
            for i in range(max(qx - cl, 0), min(qx + cl, n - 1) + 1):
                for j in range(max(qy - cl, 0), min(qy + cl, n - 1) + 1):
                    key = generateCellIDStr(i, j)
                    if key not in guaranteedNeighboringCellsSet:
                        out.add(key)
        return out

    def getNeighboringCells(self, queryRadius: float, queryPoint) -> set:
        """UniformGrid.java:261-293 (join replication); r == 0 -> every cell"""
        if queryRadius == 0:
            return self.getGirdCellsSet()
        cl = self.getCandidateNeighboringLayers(queryRadius)
        if cl <= 0:
            raise _lib.CandidateLayersError(_lib.GF_ERR_LAYERS, "candidateNeighboringLayers cannot be 0 or less")
        qx, qy = getIntCellIndices(queryPoint.gridID)
        n = self._g.n
        return {generateCellIDStr(i, j) for i in range(max(qx - cl, 0), min(qx + cl, n - 1) + 1)
                for j in range(max(qy - cl, 0), min(qy + cl, n - 1) + 1)}

    def __repr__(self):
        g = self._g
        return f"UniformGrid(n={g.n}, x=[{g.minX}, {g.maxX}], y=[{g.minY}, {g.maxY}], cellLength={g.cellLength!r})"
