"""A restatement of tRange/PointPolygonTRangeQuery.java and tFilter/PointTFilterQuery.java (windowBased,
and tRange's RealTime predicate) in plain Python over numpy float64, the reference of tests/test_trange_ref.py
and tests/test_gpu_trange.py.  contains is JTS 1.16.1 Geometry.contains(point): false unless the polygon's
envelope holds the point, then located INTERIOR -- INTERIOR of the shell, neither INTERIOR nor BOUNDARY of
any hole -- on poly_cases.ring_locate (the exact orientation sign).  No GPU, no torch, no C."""
import numpy as np

import poly_cases as PC
import traj_ref as TR


def polygon_contains(px, py, rings, exact=True):
    """bool per point: the polygon (ordered rings, shell first) contains the point"""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    minx, maxx, miny, maxy = PC.envelope(rings[0])
    out = np.zeros(len(px), bool)
    idx = np.flatnonzero((px >= minx) & (px <= maxx) & (py >= miny) & (py <= maxy))  # Envelope.contains: NaN fails
    x, y = px[idx], py[idx]
    ok = PC.ring_locate(x, y, rings[0], exact) == PC.LOC_I
    for hole in rings[1:]:
        ok &= PC.ring_locate(x, y, hole, exact) == PC.LOC_E
    out[idx] = ok
    return out


def contains_matrix(x, y, polys, exact=True):
    """[npoly, n] bool"""
    if not polys:
        return np.zeros((0, len(x)), bool)
    return np.stack([polygon_contains(x, y, rings, exact) for rings in polys])


def on_boundary(px, py, rings):
    """bool per point: on the shell's or a hole's boundary (inside the polygon's envelope)"""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    out = np.zeros(len(px), bool)
    for ring in rings:
        out |= PC.ring_locate(px, py, ring) == PC.LOC_B
    return out


def in_hole_only(px, py, rings):
    """bool per point: INTERIOR of the shell and INTERIOR of a hole"""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    sh = PC.ring_locate(px, py, rings[0]) == PC.LOC_I
    h = np.zeros(len(px), bool)
    for hole in rings[1:]:
        h |= PC.ring_locate(px, py, hole) == PC.LOC_I
    return sh & h


def cell_filter(G, x, y, polys):
    """bool per point: its cell is in the union of the polygons' gridIDsSet (the bbox cells of
    HelperClass.assignGridCellID(bBox, uGrid), integer cells, no validity test)"""
    cx, cy = G.cells(np.asarray(x, np.float64), np.asarray(y, np.float64))
    keep = np.zeros(len(cx), bool)
    for rings in polys:
        bb = PC.shell_bbox(rings)
        (x1, x2), (y1, y2) = G.cells(np.array([bb[0], bb[2]]), np.array([bb[1], bb[3]]))
        keep |= (cx >= x1) & (cx <= x2) & (cy >= y1) & (cy <= y2)
    return keep


def _csr(x, y, ts, rows):
    """rows: [(key, [indices])] -> (keys, off, x, y, ts, idx)"""
    keys = np.array([k for k, _ in rows], np.int64)
    off = np.zeros(len(rows) + 1, np.int64)
    if rows:
        off[1:] = np.cumsum([len(s) for _, s in rows])
    idx = np.array([i for _, s in rows for i in s], np.uint32)
    return keys, off, np.asarray(x)[idx], np.asarray(y)[idx], np.asarray(ts, np.int64)[idx], idx


def trange_literal(G, x, y, obj, ts, polys, use_filter=True, C=None):
    """windowBased, literally (:89-176): the window keyed by objID, trajectories in first-occurrence
    order; per point in arrival order the cell filter, then `for poly in polygons: if contains: emit the
    objID and leave the trajectory`; the hit objIDs joined back with the unfiltered window, each with all its
    points in arrival order.  C: contains_matrix(x, y, polys), computed when not given."""
    C = contains_matrix(x, y, polys) if C is None else C
    keep = cell_filter(G, x, y, polys) if use_filter else np.ones(len(x), bool)
    traj = {}
    for i, k in enumerate(np.asarray(obj, np.int64).tolist()):
        traj.setdefault(k, []).append(i)
    rows = []
    for k, seg in traj.items():
        hit = False
        for i in seg:
            if not keep[i]:
                continue
            for q in range(len(polys)):
                if C[q, i]:
                    hit = True
                    break
            if hit:
                break
        if hit:
            rows.append((k, seg))
    return _csr(x, y, ts, rows)


def trange_closed(x, y, obj, ts, polys, C=None):
    """The closed form: contains per point, any per trajectory, CSR."""
    C = contains_matrix(x, y, polys) if C is None else C
    pt = C.any(axis=0) if len(polys) else np.zeros(len(x), bool)
    keys, off, perm = TR.group_ref(obj)
    return TR.subtraj_ref(x, y, ts, keys, off, perm, pt)


def trange_points(x, y, polys, C=None):
    """RealTime (:53-87): ascending indices of the contained points"""
    C = contains_matrix(x, y, polys) if C is None else C
    return np.flatnonzero(C.any(axis=0)) if len(polys) else np.empty(0, np.int64)


def tfilter_ref(x, y, obj, ts, id_set):
    """PointTFilterQuery windowBased: the trajectories whose key is in id_set, whole; an empty set = all"""
    ids = set(int(v) for v in id_set)
    traj = {}
    for i, k in enumerate(np.asarray(obj, np.int64).tolist()):
        traj.setdefault(k, []).append(i)
    return _csr(x, y, ts, [(k, seg) for k, seg in traj.items() if not ids or k in ids])


def assert_csr_equal(got, exp):
    """keys, offsets, idx exactly; x, y by bits; ts exactly"""
    names = ("keys", "off", "x", "y", "ts", "idx")
    for name, g, e in zip(names, got, exp):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape, (name, g.shape, e.shape)
        if name in ("x", "y"):
            np.testing.assert_array_equal(g.astype(np.float64).view(np.uint64), e.astype(np.float64).view(np.uint64), err_msg=name)
        else:
            np.testing.assert_array_equal(g.astype(np.int64), e.astype(np.int64), err_msg=name)
