"""Ingest -- mirror of GeoFlink.spatialStreams.Deserialization for the CSV/TSV point stream
(Deserialization.CSVTSVToTSpatial, Deserialization.java:291-325) and the GeoJSON point stream
(Deserialization.GeoJSONToTSpatial, Deserialization.java:149-211), run on the GPU.

The reference maps each text line to a Point with String.split + Long.valueOf +
Double.valueOf and assigns its grid cell in the Point constructor (Point.java:98).  Here a whole
chunk of lines (device bytes, or host bytes uploaded once) becomes the window's SoA in one call:
gf_csv_parse (k_csv.hip) finds the lines, splits the fields with the reference's
"\\s*delim\\s*" rule, parses the numbers correctly rounded on the device and writes x, y,
objID keys (the objID field is a String, :317 -- canonical decimals are their value, any other
String goes through the device dictionary, k_objid.hip), ts and the cells (cx, cy) -- no
per-point host work.  A bad line raises ValueError naming
it (the reference's map throws NumberFormatException / IndexOutOfBoundsException).

The polygon and linestring streams (GeoJSONTo[T]SpatialPolygon, :327-458; GeoJSONTo[T]SpatialLineString,
:623-745) go through gf_geojson_parse_geoms (k_geomingest.hip): lines of GeoJSON in, a
PolygonWindow / LineStringWindow (device CSR, ready for the geometry-window operators) out.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .spatialObjects import LineStringWindow, ObjIdDict, PointWindow, PolygonWindow


class GfCsvSchema(C.Structure):
    _fields_ = [("delimiter", C.c_char), ("reserved", C.c_char * 3), ("objid_field", C.c_int32),
                ("time_field", C.c_int32), ("x_field", C.c_int32), ("y_field", C.c_int32)]


CSV_KINDS = {0: "ok", 1: "NumberFormatException", 2: "unsupported numeric literal", 3: "missing field",
             4: "empty line"}


def device_text(text, device=None):
    """bytes / bytearray / numpy uint8 -> a 16-byte-aligned device uint8 tensor (torch allocations
    are 256-B aligned); a device uint8 tensor is returned as is."""
    import torch

    if isinstance(text, torch.Tensor):
        return text
    # bytearray: a writable buffer (torch.from_numpy of a read-only array is undefined behaviour)
    arr = np.frombuffer(bytearray(text), np.uint8) if not isinstance(text, np.ndarray) else text
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


class GfGeojsonSchema(C.Structure):
    _fields_ = [("objid_property", C.c_char_p), ("time_property", C.c_char_p), ("date_format", C.c_int32),
                ("tz_offset_minutes", C.c_int32), ("value_lines", C.c_int32)]


GEOJSON_DATE_FORMATS = {None: 0, "yyyy-MM-dd HH:mm:ss": 1}


def _parse_lines(fn, schema, uGrid, text, device, capacity, objid_dict):
    import torch

    t = device_text(text, device)
    dev = t.device
    ctx = _lib.context(dev.index)
    d = objid_dict or ObjIdDict.default(dev.index)
    n = int(t.numel())
    cap = capacity if capacity is not None else max(1, n // 8 + 1)
    nout, bl, bk = C.c_int64(), C.c_int64(), C.c_int32()
    while True:
        x = torch.empty(cap, dtype=torch.float64, device=dev)
        y = torch.empty(cap, dtype=torch.float64, device=dev)
        o = torch.empty(cap, dtype=torch.int64, device=dev)
        ts = torch.empty(cap, dtype=torch.int64, device=dev)
        cx = torch.empty(cap, dtype=torch.int32, device=dev) if uGrid is not None else None
        cy = torch.empty(cap, dtype=torch.int32, device=dev) if uGrid is not None else None
        st = fn(ctx.handle, d.handle, C.c_void_p(t.data_ptr()), n, C.byref(schema),
                C.byref(uGrid.c_grid) if uGrid is not None else None, x.data_ptr(), y.data_ptr(), o.data_ptr(),
                ts.data_ptr(), cx.data_ptr() if cx is not None else None, cy.data_ptr() if cy is not None else None,
                cap, C.byref(nout), C.byref(bl), C.byref(bk))
        if st == _lib.GF_ERR_CAPACITY:
            cap = nout.value
            continue
        if st == _lib.GF_ERR_ARG and bl.value >= 0:
            raise ValueError(f"line {bl.value}: {CSV_KINDS.get(bk.value, bk.value)}")
        _lib.check(st, ctx.handle, "parse")
        break
    m = nout.value
    w = PointWindow(x[:m], y[:m], o[:m], ts[:m], objid_dict=d)
    if cx is not None:
        w.extra["cx"], w.extra["cy"] = cx[:m], cy[:m]
    return w


def _parse_geoms(kind, schema, text, device, objid_dict, fn="gf_geojson_parse_geoms"):
    """gf_geojson_parse_geoms / gf_wkt_parse_geoms: one sizing call (zero capacities), then the
    exact-size call."""
    import torch

    t = device_text(text, device)
    dev = t.device
    ctx = _lib.context(dev.index)
    d = objid_dict or ObjIdDict.default(dev.index)
    poly = kind == _lib.GEOM_POLYGON
    nobj, nr, nv, bl, bk = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
    ptr = lambda a: a.data_ptr() if a is not None else None  # noqa: E731

    def call(out):
        st = getattr(_lib.lib(), fn)(ctx.handle, d.handle, C.c_void_p(t.data_ptr()), int(t.numel()), C.byref(schema),
                                     C.byref(out), C.byref(nobj), C.byref(nr), C.byref(nv), C.byref(bl), C.byref(bk))
        if st == _lib.GF_ERR_ARG and bl.value >= 0:
            raise ValueError(f"line {bl.value}: {CSV_KINDS.get(bk.value, bk.value)}")
        return st

    st = call(_lib.GfGeomsOut(kind, 0, 0, 0, None, None, None, None, None, None))  # the sizes
    if st != _lib.GF_ERR_CAPACITY:
        _lib.check(st, ctx.handle, fn)
    n, r, v = nobj.value, nr.value, nv.value
    ro = torch.zeros(n + 1, dtype=torch.int32, device=dev) if poly else None
    vo = torch.zeros((r if poly else n) + 1, dtype=torch.int32, device=dev)
    vx = torch.empty(v, dtype=torch.float64, device=dev)
    vy = torch.empty(v, dtype=torch.float64, device=dev)
    o = torch.empty(n, dtype=torch.int64, device=dev)
    ts = torch.empty(n, dtype=torch.int64, device=dev)
    if n > 0:  # (empty text: the zeroed offsets are the empty window)
        _lib.check(call(_lib.GfGeomsOut(kind, n, r, v, ptr(ro), ptr(vo), ptr(vx), ptr(vy), ptr(o), ptr(ts))),
                   ctx.handle, fn)
    cls = PolygonWindow if poly else LineStringWindow
    return cls(int(kind), ro, vo, vx, vy, o, ts, nobj.value, objid_dict=d)


class _GeoJSONToGeoms:
    """The four geometry-stream deserializers: lines of GeoJSON -> a geometry window on the GPU
    (gf_geojson_parse_geoms; the contract is in include/geoflink_hip.h).  The lines, the number
    rule and the properties are GeoJSONToTSpatial's; the object is the taken Polygon's rings in
    createPolygon order / the LineString's positions, a Multi*'s first member only."""

    kind = None

    def __init__(self, uGrid=None, dateFormat=None, propertyTimeStamp=None, propertyObjID=None, tz_offset_minutes=0,
                 value_lines=False):
        if dateFormat not in GEOJSON_DATE_FORMATS:
            raise ValueError(f"dateFormat {dateFormat!r}: supported {list(GEOJSON_DATE_FORMATS)}")
        self.uGrid = uGrid
        self._names = (propertyObjID.encode() if propertyObjID else None,
                       propertyTimeStamp.encode() if propertyTimeStamp else None)
        self.schema = GfGeojsonSchema(self._names[0], self._names[1], GEOJSON_DATE_FORMATS[dateFormat],
                                      int(tz_offset_minutes), int(bool(value_lines)))

    def parse(self, text, device=None, objid_dict: ObjIdDict = None):
        return _parse_geoms(self.kind, self.schema, text, device, objid_dict)


class _GeoJSONToGeomsPlain(_GeoJSONToGeoms):
    """The non-T deserializers: no properties are read (objID null, ts 0)."""

    def __init__(self, uGrid=None, value_lines=False):
        super().__init__(uGrid, None, None, None, 0, value_lines)


class GfWktSchema(C.Structure):
    _fields_ = [("delimiter", C.c_char), ("reserved", C.c_char * 3), ("date_format", C.c_int32),
                ("tz_offset_minutes", C.c_int32)]


class _WKTToGeoms:
    """The four WKT geometry-stream deserializers: lines holding a WKT geometry -> a geometry window
    on the GPU (gf_wkt_parse_geoms; the contract is in include/geoflink_hip.h).  The T variants
    split the line by `delimiter` for the objID (field 0) and the time (the last field that parses
    as `dateFormat`)."""

    kind = None

    def __init__(self, uGrid=None, dateFormat=None, delimiter=",", tz_offset_minutes=0):
        if dateFormat not in GEOJSON_DATE_FORMATS:
            raise ValueError(f"dateFormat {dateFormat!r}: supported {list(GEOJSON_DATE_FORMATS)}")
        if len(delimiter) != 1 or delimiter in "\0\"":
            raise ValueError("single-character delimiters only (not '\"': it is removed before the split)")
        self.uGrid = uGrid
        self.schema = GfWktSchema(delimiter.encode(), b"\0\0\0", GEOJSON_DATE_FORMATS[dateFormat],
                                  int(tz_offset_minutes))

    def parse(self, text, device=None, objid_dict: ObjIdDict = None):
        return _parse_geoms(self.kind, self.schema, text, device, objid_dict, "gf_wkt_parse_geoms")


class _WKTToGeomsPlain(_WKTToGeoms):
    """The non-T deserializers: no field is read (objID null, ts 0)."""

    def __init__(self, uGrid=None):
        self.uGrid = uGrid
        self.schema = GfWktSchema(b"\0", b"\0\0\0", 0, 0)


class _WKTToPoints:
    """WKTToSpatial / WKTToTSpatial: both maps build Point(x, y, uGrid) from the line's POINT, so
    objID is null and ts 0 on every line (gf_wkt_parse_points)."""

    def __init__(self, uGrid=None):
        self.uGrid = uGrid

    def parse(self, text, device=None, objid_dict: ObjIdDict = None) -> PointWindow:
        import torch

        t = device_text(text, device)
        dev = t.device
        ctx = _lib.context(dev.index)
        d = objid_dict or ObjIdDict.default(dev.index)
        n = int(t.numel())
        g = self.uGrid
        cap = max(1, n // 16 + 1)
        nout, bl, bk = C.c_int64(), C.c_int64(), C.c_int32()
        while True:
            x = torch.empty(cap, dtype=torch.float64, device=dev)
            y = torch.empty(cap, dtype=torch.float64, device=dev)
            o = torch.empty(cap, dtype=torch.int64, device=dev)
            ts = torch.empty(cap, dtype=torch.int64, device=dev)
            cx = torch.empty(cap, dtype=torch.int32, device=dev) if g is not None else None
            cy = torch.empty(cap, dtype=torch.int32, device=dev) if g is not None else None
            st = _lib.lib().gf_wkt_parse_points(
                ctx.handle, C.c_void_p(t.data_ptr()), n, C.byref(g.c_grid) if g is not None else None, x.data_ptr(),
                y.data_ptr(), o.data_ptr(), ts.data_ptr(), cx.data_ptr() if g is not None else None,
                cy.data_ptr() if g is not None else None, cap, C.byref(nout), C.byref(bl), C.byref(bk))
            if st == _lib.GF_ERR_CAPACITY:
                cap = nout.value
                continue
            if st == _lib.GF_ERR_ARG and bl.value >= 0:
                raise ValueError(f"line {bl.value}: {CSV_KINDS.get(bk.value, bk.value)}")
            _lib.check(st, ctx.handle, "gf_wkt_parse_points")
            break
        m = nout.value
        w = PointWindow(x[:m], y[:m], o[:m], ts[:m], objid_dict=d)
        if g is not None:
            w.extra["cx"], w.extra["cy"] = cx[:m], cy[:m]
        return w


class Deserialization:
    class WKTToSpatial(_WKTToPoints):
        """WKTToSpatial(uGrid) (Deserialization.java:214-232) -> PointWindow."""

    class WKTToTSpatial(_WKTToPoints):
        """WKTToTSpatial(uGrid, dateFormat, delimiter) (Deserialization.java:261-288) -> PointWindow; the
        reference's map reads neither its date format nor its delimiter."""

        def __init__(self, uGrid=None, dateFormat=None, delimiter=","):
            super().__init__(uGrid)

    class WKTToSpatialPolygon(_WKTToGeomsPlain):
        """WKTToSpatialPolygon(uGrid) (Deserialization.java:461-490) -> PolygonWindow."""
        kind = _lib.GEOM_POLYGON

    class WKTToTSpatialPolygon(_WKTToGeoms):
        """WKTToTSpatialPolygon(uGrid, dateFormat, delimiter) (Deserialization.java:524-586) -> PolygonWindow."""
        kind = _lib.GEOM_POLYGON

    class WKTToSpatialLineString(_WKTToGeomsPlain):
        """WKTToSpatialLineString(uGrid) (Deserialization.java:748-776) -> LineStringWindow."""
        kind = _lib.GEOM_LINESTRING

    class WKTToTSpatialLineString(_WKTToGeoms):
        """WKTToTSpatialLineString(uGrid, dateFormat, delimiter) (Deserialization.java:778-835) ->
        LineStringWindow."""
        kind = _lib.GEOM_LINESTRING

    # ---- the reference's dispatchers (Deserialization.java:47-115, :588-621): the map for an inputType ----
    @staticmethod
    def PointStream(inputType, delimiter=",", csvTsvSchemaAttr=(0, 1, 2, 3), uGrid=None):
        if inputType == "WKT":
            return Deserialization.WKTToSpatial(uGrid)
        raise ValueError("Not yet support")  # GeoJSONToSpatial / CSVTSVToSpatial: the non-T point maps

    @staticmethod
    def TrajectoryStream(inputType, dateFormat=None, delimiter=",", csvTsvSchemaAttr=(0, 1, 2, 3),
                         propertyTimeStamp=None, propertyObjID=None, uGrid=None):
        if inputType == "GeoJSON":
            return Deserialization.GeoJSONToTSpatial(uGrid, dateFormat, propertyTimeStamp, propertyObjID)
        if inputType == "WKT":
            return Deserialization.WKTToTSpatial(uGrid, dateFormat, delimiter)
        return Deserialization.CSVTSVToTSpatial(uGrid, dateFormat, delimiter, csvTsvSchemaAttr)

    @staticmethod
    def PolygonStream(inputType, uGrid=None):
        if inputType == "GeoJSON":
            return Deserialization.GeoJSONToSpatialPolygon(uGrid)
        if inputType == "WKT":
            return Deserialization.WKTToSpatialPolygon(uGrid)
        raise ValueError(f"inputType : {inputType} is not support")

    @staticmethod
    def TrajectoryStreamPolygon(inputType, dateFormat=None, delimiter=",", propertyTimeStamp=None, propertyObjID=None,
                                uGrid=None):
        if inputType == "GeoJSON":
            return Deserialization.GeoJSONToTSpatialPolygon(uGrid, dateFormat, propertyTimeStamp, propertyObjID)
        if inputType == "WKT":
            return Deserialization.WKTToTSpatialPolygon(uGrid, dateFormat, delimiter)
        raise ValueError(f"inputType : {inputType} is not support")

    @staticmethod
    def LineStringStream(inputType, uGrid=None):
        if inputType == "GeoJSON":
            return Deserialization.GeoJSONToSpatialLineString(uGrid)
        if inputType == "WKT":
            return Deserialization.WKTToSpatialLineString(uGrid)
        raise ValueError(f"inputType : {inputType} is not support")

    @staticmethod
    def TrajectoryStreamLineString(inputType, dateFormat=None, delimiter=",", propertyTimeStamp=None,
                                   propertyObjID=None, uGrid=None):
        if inputType == "GeoJSON":
            return Deserialization.GeoJSONToTSpatialLineString(uGrid, dateFormat, propertyTimeStamp, propertyObjID)
        if inputType == "WKT":
            return Deserialization.WKTToTSpatialLineString(uGrid, dateFormat, delimiter)
        raise ValueError(f"inputType : {inputType} is not support")

    class GeoJSONToTSpatialPolygon(_GeoJSONToGeoms):
        """GeoJSONToTSpatialPolygon(uGrid, dateFormat, propertyTimeStamp, propertyObjID)
        (Deserialization.java:389-458) -> PolygonWindow."""
        kind = _lib.GEOM_POLYGON

    class GeoJSONToSpatialPolygon(_GeoJSONToGeomsPlain):
        """GeoJSONToSpatialPolygon(uGrid) (Deserialization.java:327-387) -> PolygonWindow."""
        kind = _lib.GEOM_POLYGON

    class GeoJSONToTSpatialLineString(_GeoJSONToGeoms):
        """GeoJSONToTSpatialLineString(uGrid, dateFormat, propertyTimeStamp, propertyObjID)
        (Deserialization.java:683-745) -> LineStringWindow."""
        kind = _lib.GEOM_LINESTRING

    class GeoJSONToSpatialLineString(_GeoJSONToGeomsPlain):
        """GeoJSONToSpatialLineString(uGrid) (Deserialization.java:623-681) -> LineStringWindow."""
        kind = _lib.GEOM_LINESTRING

    class GeoJSONToTSpatial:
        """GeoJSONToTSpatial(uGrid, dateFormat, propertyTimeStamp, propertyObjID)
        (Deserialization.java:149-211) over lines of GeoJSON, run on the GPU (gf_geojson_parse):
        one Kafka key/value record ({"key": .., "value": ..}, the ObjectNode the map receives) per
        line, or with value_lines=True the record's value itself (a Feature as the reference's
        Serialization writes it).  dateFormat: None (the time property is integer milliseconds)
        or "yyyy-MM-dd HH:mm:ss" in a fixed UTC offset `tz_offset_minutes` (the reference JVM's
        default zone).  A feature without the objID property has objID None (key OBJID_NULL)."""

        def __init__(self, uGrid=None, dateFormat=None, propertyTimeStamp=None, propertyObjID=None,
                     tz_offset_minutes=0, value_lines=False):
            if dateFormat not in GEOJSON_DATE_FORMATS:
                raise ValueError(f"dateFormat {dateFormat!r}: supported {list(GEOJSON_DATE_FORMATS)}")
            self.uGrid = uGrid
            self._names = (propertyObjID.encode() if propertyObjID else None,
                           propertyTimeStamp.encode() if propertyTimeStamp else None)
            self.schema = GfGeojsonSchema(self._names[0], self._names[1], GEOJSON_DATE_FORMATS[dateFormat],
                                          int(tz_offset_minutes), int(bool(value_lines)))

        def parse(self, text, device=None, capacity=None, objid_dict: ObjIdDict = None) -> PointWindow:
            return _parse_lines(_lib.lib().gf_geojson_parse, self.schema, self.uGrid, text, device, capacity,
                                objid_dict)

    class CSVTSVToTSpatial:
        """CSVTSVToTSpatial(uGrid, dateFormat, delimiter, csvTsvSchemaAttr) -- csvTsvSchemaAttr
        lists the field indices of objID, timestamp, x, y (Deserialization.java:314-322).
        dateFormat is unused by the reference's map (the time field is Long.valueOf)."""

        def __init__(self, uGrid=None, dateFormat=None, delimiter=",", csvTsvSchemaAttr=(0, 1, 2, 3)):
            if len(delimiter) != 1:
                raise ValueError("single-character delimiters only")
            self.uGrid = uGrid
            self.delimiter = delimiter
            a = list(csvTsvSchemaAttr)
            self.schema = GfCsvSchema(delimiter.encode(), b"\0\0\0", a[0], a[1], a[2], a[3])

        def parse(self, text, device=None, capacity=None, objid_dict: ObjIdDict = None) -> PointWindow:
            """All lines of `text` -> one PointWindow (extra: cx, cy when a grid is set).  objID
            Strings become keys of `objid_dict` (default: the device context's dictionary)."""
            return _parse_lines(_lib.lib().gf_csv_parse_dict, self.schema, self.uGrid, text, device, capacity,
                                objid_dict)
