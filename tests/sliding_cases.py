"""Streams, batch cuts and gaps for the sliding pane engines (CPU helpers, nothing here touches the GPU).

A stream is a sequence of panes of gcd(size, slide) ms; each pane gets a chosen number of points within
r of QPOINT (distinct objIDs, some repeated from the pane before) and of points farther than r, drawn
from oracle.java_random_points over BEIJING, plus PLACED points at dyadic offsets from QPOINT.  The
placed points make an off-by-one at a pane edge visible in the record, not only in the membership:

  end / start   for a window end b and a window start b, the two closest points of the whole stream
                neighbourhood carry ts = b - 1 and ts = b (different objIDs, 2^-30 and 2^-29 from q);
  dup_closer    one objID in two panes of one window, the later one closer;
  dup_tie       one objID at the very same coordinates in two panes;
  straddle      k - 1 placed objIDs, then two different objIDs at one location in the window's first
                and last pane: they sit at ranks k - 1 and k, the smaller objID is the record's last.

Layout of a stream, in panes (W = panes per window, S = panes per slide, L = W + S + 2):
  5 L light panes (2 neighbours each, the very first k + 2) carrying the placed points, L apart;
  W + S rich panes of ~0.6 k neighbours and one of k + 2: windows where only the merge reaches k;
  L far-only panes, one lone pane of min(k - 1, 3) neighbours, L far-only panes: zero and short records;
  W + S empty panes: a window that must not fire;
  L light panes.
"""
from collections import namedtuple

import numpy as np

from conftest import BEIJING, QPOINT

R_KNN = 0.5
R_RANGE = 0.05
R_POLY = 0.01
ORIGINS = {"zero": 0, "negative": -7_500, "epoch": 1_700_000_000_123, "deep": -(1 << 40) + 17}
GEOMETRIES = [(1000, 1000), (1000, 3000), (3000, 2000), (7000, 2000), (63000, 2000), (64000, 1000), (6400, 100)]
# two query polygons near QPOINT: a square holding it and a triangle 0.1 east of it
POLYGONS = [
    [[(QPOINT[0] - 0.03, QPOINT[1] - 0.03), (QPOINT[0] + 0.03, QPOINT[1] - 0.03), (QPOINT[0] + 0.03, QPOINT[1] + 0.03),
      (QPOINT[0] - 0.03, QPOINT[1] + 0.03), (QPOINT[0] - 0.03, QPOINT[1] - 0.03)]],
    [[(QPOINT[0] + 0.10, QPOINT[1]), (QPOINT[0] + 0.14, QPOINT[1]), (QPOINT[0] + 0.12, QPOINT[1] + 0.03),
      (QPOINT[0] + 0.10, QPOINT[1])]],
]

Stream = namedtuple("Stream", "x y obj ts placed size slide pane W S p0 npanes")
Placed = namedtuple("Placed", "kind obj ts window note")   # window = (start, end) the point was placed for


def geometry(size, slide):
    pane = int(np.gcd(size, slide))
    return pane, size // pane, slide // pane


def expected_windows(ts, size, slide):
    """Flink's assignment, brute force: window [s, s + size), s a multiple of slide, fires iff it holds a
    timestamp; in order of window end.  Integer floor arithmetic only (negative ts, slide > size)."""
    ts = np.unique(np.asarray(ts, np.int64))
    if len(ts) == 0:
        return []
    lo, hi = int(ts[0]), int(ts[-1])
    out = []
    s = ((lo - size) // slide) * slide       # the last multiple of slide <= lo - size: holds nothing
    while s <= hi:
        a, b = np.searchsorted(ts, [s, s + size], side="left")
        if b > a:
            out.append((s, s + size))
        s += slide
    return out


def _aligned(p, S, rem=0):
    """The first pane index >= p with index = rem (mod S)."""
    return p + (rem - p) % S


def build_stream(oracle_mod, size, slide, origin, k, seed=1):
    pane, W, S = geometry(size, slide)
    L = W + S + 2
    p0 = origin // pane
    mN = max(1, (6 * k) // 10) if k > 1 else 1
    kinds = []                                  # (neighbours, far points) per pane
    kinds += [(min(2, max(k - 1, 1)), 3)] * (5 * L)
    kinds[0] = (k + 2, 3)                       # the stream opens with a full pane: its windows reach before the stream
    rich0 = len(kinds)
    kinds += [(mN, 3)] * (W + S)
    kinds[rich0 + 1] = (k + 2, 3)
    kinds += [(0, 4)] * L
    lone = _aligned(p0 + len(kinds), S) - p0
    kinds += [(0, 4)] * (lone - len(kinds))
    kinds += [(min(max(k - 1, 0), 3), 2)]
    kinds += [(0, 4)] * L
    kinds += [(0, 0)] * (W + S)
    kinds += [(2, 3)] * L
    npanes = len(kinds)

    need_near = sum(m for m, _ in kinds)
    need_far = sum(f for _, f in kinds)
    npool = 12 * need_near + 6 * need_far + 4096
    px, py = oracle_mod.java_random_points(seed, npool, *BEIJING)
    d = np.hypot(px - QPOINT[0], py - QPOINT[1])
    near = np.flatnonzero((d > 2.0 ** -6) & (d < 0.9 * R_KNN))
    far = np.flatnonzero(d > 1.1 * R_KNN)
    assert len(near) >= need_near and len(far) >= need_far
    rng = np.random.default_rng(seed)
    xs, ys, os_, tss = [], [], [], []
    ni = fi = 0
    next_obj = 1000
    prev_near_obj = []
    for j, (m, f) in enumerate(kinds):
        lo = (p0 + j) * pane
        idx = np.concatenate([near[ni:ni + m], far[fi:fi + f]])
        ni += m
        fi += f
        obj = np.arange(next_obj, next_obj + m + f, dtype=np.int64)
        next_obj += m + f
        # every fifth neighbour repeats an objID of the pane before: windows dedupe across panes
        for t in range(0, min(m, len(prev_near_obj)), 5):
            obj[t] = prev_near_obj[t]
        # the far points repeat objIDs freely
        obj[m:] = 500 + (np.arange(f) + j) % 7
        prev_near_obj = obj[:m].tolist()
        xs.append(px[idx]); ys.append(py[idx]); os_.append(obj)
        tss.append(lo + np.sort(rng.integers(0, pane, m + f)).astype(np.int64))

    placed = []
    ex, ey, eo, et = [], [], [], []
    nobj = [10_000_000]

    def put(kind, dx, dy, ts, window=None, obj=None, note=""):
        if obj is None:
            obj = nobj[0]
            nobj[0] += 1
        ex.append(QPOINT[0] + dx); ey.append(QPOINT[1] + dy); eo.append(obj); et.append(int(ts))
        placed.append(Placed(kind, obj, int(ts), window, note))
        return obj

    e1, e2 = 2.0 ** -30, 2.0 ** -29
    # a window END at b: pane p - 1 closes a window
    p = _aligned(p0 + L, S, W % S)
    b = p * pane
    assert (b - size) % slide == 0
    put("end", e1, 0.0, b - 1, (b - size, b), note="rank 0 of the window ending at b")
    put("end", e2, 0.0, b, None, note="must stay out of the window ending at b")
    # a window START at b
    p = _aligned(p0 + 2 * L, S)
    b = p * pane
    assert b % slide == 0
    put("start", e1, 0.0, b - 1, None, note="must stay out of the window starting at b")
    put("start", e2, 0.0, b, (b, b + size), note="rank 0 of the window starting at b")
    # one objID twice in one window, and one objID twice at one location
    p = _aligned(p0 + 3 * L, S)
    q = p + (1 if W > 1 else 0)
    win = (p * pane, p * pane + size)
    o = put("dup_closer", 2.0 ** -20, 0.0, p * pane + pane // 3, win, note="farther")
    put("dup_closer", 2.0 ** -21, 0.0, q * pane + pane // 2, win, obj=o, note="closer")
    o = put("dup_tie", 0.0, -2.0 ** -19, p * pane + pane // 4, win)
    put("dup_tie", 0.0, -2.0 ** -19, q * pane + (3 * pane) // 4, win, obj=o)
    # two objIDs at one location on ranks k - 1 and k, from the window's first and last pane
    p = _aligned(p0 + 4 * L, S)
    win = (p * pane, p * pane + size)
    for t in range(k - 1):
        put("filler", (64 + t) * 2.0 ** -24, 0.0, (p + t % W) * pane + (t * 37) % pane, win)
    put("straddle", 0.0, 2.0 ** -12, (p + W - 1) * pane + pane // 2, win, note="smaller objID: rank k - 1")
    put("straddle", 0.0, 2.0 ** -12, p * pane + pane // 2, win, note="larger objID: rank k, left out")

    x = np.concatenate(xs + [np.array(ex)])
    y = np.concatenate(ys + [np.array(ey)])
    obj = np.concatenate(os_ + [np.array(eo, np.int64)])
    ts = np.concatenate(tss + [np.array(et, np.int64)])
    order = np.argsort(ts, kind="stable")
    return Stream(x[order], y[order], obj[order], ts[order], placed, size, slide, pane, W, S, p0, npanes)


_STREAMS = {}


def stream(oracle_mod, size, slide, origin, k, seed=1):
    key = (size, slide, origin, k, seed)
    if key not in _STREAMS:
        _STREAMS[key] = build_stream(oracle_mod, size, slide, origin, k, seed)
    return _STREAMS[key]


def shifted(s, by):
    return s._replace(ts=s.ts + by, p0=s.p0 + by // s.pane,
                      placed=[p._replace(ts=p.ts + by, window=p.window and (p.window[0] + by, p.window[1] + by))
                              for p in s.placed])


def subset(s, keep):
    return s._replace(x=s.x[keep], y=s.y[keep], obj=s.obj[keep], ts=s.ts[keep])


# ---------------------------------------------------------------------------------------------
# references: the oracle from scratch on each window's points, computed once per stream
# ---------------------------------------------------------------------------------------------
_REF = {}


def window_masks(s):
    for a, b in expected_windows(s.ts, s.size, s.slide):
        lo, hi = np.searchsorted(s.ts, [a, b], side="left")
        yield (a, b), slice(int(lo), int(hi))


def _key(s, *rest):
    return (s.ts.tobytes(), s.obj.tobytes(), s.x.tobytes(), s.size, s.slide) + rest


def knn_reference(oracle_mod, s, k, grid_n=100, r=R_KNN):
    """[((start, end), status, objID, dist, idx)] for every window that fires."""
    key = _key(s, "knn", k, grid_n, r)
    if key not in _REF:
        og = oracle_mod.grid(grid_n, *BEIJING)
        out = []
        for w, m in window_masks(s):
            st, o, d, i = oracle_mod.knn(og, s.x[m], s.y[m], s.obj[m], QPOINT[0], QPOINT[1], r, k)
            out.append((w, st, o, d, i))
        _REF[key] = out
    return _REF[key]


def range_reference(oracle_mod, s, poly, grid_n=100):
    key = _key(s, "range", poly, grid_n)
    if key not in _REF:
        og = oracle_mod.grid(grid_n, *BEIJING)
        P = oracle_mod.Polygons(POLYGONS) if poly else None
        out = []
        for w, m in window_masks(s):
            if poly:
                h = oracle_mod.range_ppoly(og, s.x[m], s.y[m], P, R_POLY)
            else:
                h = oracle_mod.range_pp(og, s.x[m], s.y[m], [QPOINT[0]], [QPOINT[1]], R_RANGE)
            out.append((w, np.array(h, np.int64)))
        _REF[key] = out
    return _REF[key]


def pane_neighbours(oracle_mod, s, k, grid_n=100, r=R_KNN):
    """{pane index: distinct objIDs within r among the pane's points} (the oracle with k = the pane's size)."""
    og = oracle_mod.grid(grid_n, *BEIJING)
    out = {}
    panes = np.floor_divide(s.ts, s.pane)
    for p in np.unique(panes):
        m = panes == p
        st, o, _, _ = oracle_mod.knn(og, s.x[m], s.y[m], s.obj[m], QPOINT[0], QPOINT[1], r, int(m.sum()))
        assert st == 0
        out[int(p)] = len(o)
    return out


# ---------------------------------------------------------------------------------------------
# cuts: batch boundaries [0, ..., n]
# ---------------------------------------------------------------------------------------------
def pane_starts(s):
    """Element offset of every non-empty pane's first point."""
    panes = np.floor_divide(s.ts, s.pane)
    return np.flatnonzero(np.r_[True, panes[1:] != panes[:-1]])


def _cuts(s, inner):
    n = len(s.ts)
    return [0] + sorted({int(c) for c in inner if 0 < int(c) < n}) + [n]


def cut_whole(s):
    return [0, len(s.ts)]


def cut_on_panes(s):
    return _cuts(s, pane_starts(s)[1::3])


def cut_mid(s):
    """The largest pane is cut at two inner points (it spans 3 batches); a few cuts elsewhere."""
    st = np.r_[pane_starts(s), len(s.ts)]
    j = int(np.argmax(np.diff(st)))
    a, b = int(st[j]), int(st[j + 1])
    assert b - a >= 3
    return _cuts(s, [a + (b - a) // 3, a + 2 * (b - a) // 3, len(s.ts) // 5, (4 * len(s.ts)) // 5])


def cut_singles(s, run=50):
    """About 50 one-point batches that start inside a pane and run across its end."""
    st = pane_starts(s)
    j = len(st) // 2
    lo = max(1, int(st[j]) - run // 2)
    return _cuts(s, range(lo, lo + run))


def cut_odd_even(s):
    """Cuts after which pane slices start at odd and at even offsets of their batch."""
    st = pane_starts(s)
    inner = []
    for j in range(1, len(st) - 1, 4):
        inner.append(int(st[j]) - (1 if (j // 4) % 2 else 2))
    return _cuts(s, inner)


CUTS = {"whole": cut_whole, "on_panes": cut_on_panes, "mid": cut_mid, "singles": cut_singles, "odd_even": cut_odd_even}


def slice_parities(s, cuts):
    """Parities of (pane slice start - batch start) over every pane slice that starts inside a batch."""
    out = set()
    st = pane_starts(s)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        for p in st[(st > lo) & (st < hi)]:
            out.add(int(p - lo) % 2)
    return out


def max_batches_per_pane(s, cuts):
    st = np.r_[pane_starts(s), len(s.ts)]
    c = np.array(cuts[1:-1])
    return max(1 + int(np.count_nonzero((c > a) & (c < b))) for a, b in zip(st[:-1], st[1:]))


# ---------------------------------------------------------------------------------------------
# gaps: all points of some consecutive panes removed
# ---------------------------------------------------------------------------------------------
def gap_lengths(s):
    return {"bridge": s.W - 1, "exact": s.W, "ring": 2 * s.W + s.S + 3}


def with_gap(s, kind, straddle):
    """The stream without the points of `gap_lengths(s)[kind]` panes, from a window start in the rich run
    on, and cuts: the gap lies inside one batch, or a cut falls exactly on it (the batch before ends with
    the last point before the gap)."""
    npanes = gap_lengths(s)[kind]
    first = _aligned(s.p0 + 5 * (s.W + s.S + 2) + 1, s.S)      # in the rich run, on a window start
    keep = ~((s.ts >= first * s.pane) & (s.ts < (first + npanes) * s.pane))
    g = subset(s, keep)
    at = int(np.searchsorted(g.ts, first * s.pane, side="left"))  # the first point after the gap
    n = len(g.ts)
    assert 8 < at < n - 8
    cuts = [0, at, n] if straddle else [0, at - 5, at + 5, n]
    return g, cuts, (first, npanes)


def batches_of(s, cuts):
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        yield s.x[lo:hi], s.y[lo:hi], s.obj[lo:hi], s.ts[lo:hi]


# ---------------------------------------------------------------------------------------------
# the cases the CPU conditions and the GPU runs share: (size, slide, origin name, k)
# ---------------------------------------------------------------------------------------------
MATRIX_K = 5
MATRIX_ORIGINS = ("zero", "negative", "epoch")
MATRIX = [(sz, sl, o, MATRIX_K) for sz, sl in GEOMETRIES for o in MATRIX_ORIGINS]
CUT_GEOMETRIES = [(3000, 2000), (5000, 3000)]
CUT_K = 7
K_GEOMETRIES = [(3000, 1000), (5000, 3000)]
KS = (1, 127, 128, 129, 256, 257, 512, 513)
K_CASES = [(sz, sl, "zero", k) for sz, sl in K_GEOMETRIES for k in KS]
OVERFLOW_KS = (7, 300)
KNN_CASES = (MATRIX + [(sz, sl, "negative", CUT_K) for sz, sl in CUT_GEOMETRIES] + K_CASES
             + [(3000, 1000, "negative", k) for k in OVERFLOW_KS] + [(3000, 1000, "zero", MATRIX_K)])


def case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-k{c[3]}"


def case_stream(oracle_mod, c):
    return stream(oracle_mod, c[0], c[1], ORIGINS[c[2]], c[3])
