"""CPU: the helpers of tests/sliding_cases.py, and the CONDITIONS its streams must meet for the GPU
tests of the sliding pane engines (test_gpu_sliding_edges.py) to mean what they claim -- every one
shown from the oracle alone."""
import numpy as np
import pytest

import sliding_cases as SC


@pytest.mark.parametrize("size,slide", SC.GEOMETRIES + SC.CUT_GEOMETRIES[1:] + SC.K_GEOMETRIES[:1] + [(65000, 1000)])
@pytest.mark.parametrize("origin", list(SC.ORIGINS.values()))
def test_expected_windows_is_flinks_assignment(size, slide, origin):
    """expected_windows == the union of SlidingWindows.assign_windows over the timestamps, in order of
    window end, and == the windows the pane walk closes (closes / window_of_last_pane) that hold a point."""
    from spatialflink_amd.windows import SlidingWindows

    g = SlidingWindows(size, slide)
    rng = np.random.default_rng(size + slide)
    span = 3 * (size + slide)
    ts = origin + np.sort(np.r_[rng.integers(0, span // 3, 40), rng.integers(span - size // 2, span, 25)])
    pane = g.pane
    b = (origin // pane + 2) * pane
    ts = np.sort(np.r_[ts, b - 1, b, b, origin + span + 2 * (size + slide)]).astype(np.int64)
    exp = SC.expected_windows(ts, size, slide)
    starts = sorted({s for t in ts.tolist() for s in g.assign_windows(t)})
    assert exp == [(s, s + size) for s in starts]
    walk = []
    for p in range(int(ts[0]) // pane, int(ts[-1]) // pane + g.panes_per_window + g.panes_per_slide + 1):
        if g.closes(p):
            s, e = g.window_of_last_pane(p)
            if np.any((ts >= s) & (ts < e)):
                walk.append((s, e))
    assert exp == walk
    if slide > size:  # some points belong to no window
        assert any(not g.assign_windows(t) for t in ts.tolist())


@pytest.mark.parametrize("case", SC.KNN_CASES, ids=SC.case_id)
def test_knn_stream_conditions(oracle_mod, case):
    size, slide, _, k = case
    s = SC.case_stream(oracle_mod, case)
    assert np.all(np.diff(s.ts) >= 0) and len(s.ts) <= 24_000
    ref = SC.knn_reference(oracle_mod, s, k)
    assert [w for w, *_ in ref] == SC.expected_windows(s.ts, size, slide)
    assert all(st == 0 for _, st, *_ in ref)
    counts = [len(o) for _, _, o, _, _ in ref]
    assert k in counts                               # a full record
    assert any(c < k for c in counts)                # a short one
    assert 0 in counts                               # a fired window with points, none within r
    # an empty window does not fire
    fired = {w for w, *_ in ref}
    every = {(a, a + size) for a in range((int(s.ts[0]) // slide) * slide, int(s.ts[-1]), slide)}
    assert every - fired
    if s.p0 < 0:
        assert s.ts[0] < 0 < s.ts[-1] or s.ts[-1] < 0  # negative pane indices
    # a window where the merge decides: k or more distinct neighbours, no single pane with k (a one-pane
    # window has no merge, and with k = 1 a window with a neighbour has a pane with one)
    if s.W > 1 and k > 1:
        per = SC.pane_neighbours(oracle_mod, s, k)
        decided = 0
        for (a, b), _, o, _, _ in ref:
            if len(o) == k and all(per.get(p, 0) < k for p in range(a // s.pane, b // s.pane)):
                decided += 1
        assert decided > 0
    # the placed edge points are rank 0 of their windows, the other of each pair is not in them
    by = {w: (o, d, i) for w, _, o, d, i in ref}
    for kind in ("end", "start"):
        inside = [p for p in s.placed if p.kind == kind and p.window]
        outside = [p for p in s.placed if p.kind == kind and not p.window]
        assert len(inside) == 1 and len(outside) == 1
        o, d, i = by[inside[0].window]
        assert o[0] == inside[0].obj and outside[0].obj not in o
        lo = np.searchsorted(s.ts, inside[0].window[0])
        assert s.ts[lo + i[0]] == inside[0].ts
        assert abs(inside[0].ts - outside[0].ts) == 1
        assert (inside[0].ts if kind == "start" else outside[0].ts) % s.pane == 0
    # one objID in two panes: the closer (later) one is reported, with its own index
    far_, close_ = [p for p in s.placed if p.kind == "dup_closer"]
    o, d, i = by[far_.window]
    lo = np.searchsorted(s.ts, far_.window[0])
    j = int(np.flatnonzero(o == far_.obj)[0]) if far_.obj in o else None
    if k >= 4:
        assert j is not None
    if j is not None:
        assert s.ts[lo + i[j]] == close_.ts and (s.W == 1 or close_.ts // s.pane != far_.ts // s.pane)
    # two objIDs at one location on ranks k - 1 and k
    a_, b_ = [p for p in s.placed if p.kind == "straddle"]
    o, d, i = by[a_.window]
    assert len(o) == k and o[-1] == min(a_.obj, b_.obj) and max(a_.obj, b_.obj) not in o
    assert s.W == 1 or a_.ts // s.pane != b_.ts // s.pane


@pytest.mark.parametrize("case", SC.MATRIX + [(sz, sl, "negative", SC.CUT_K) for sz, sl in SC.CUT_GEOMETRIES],
                         ids=SC.case_id)
@pytest.mark.parametrize("poly", [False, True])
def test_range_stream_conditions(oracle_mod, case, poly):
    s = SC.case_stream(oracle_mod, case)
    ref = SC.range_reference(oracle_mod, s, poly)
    assert any(len(h) == 0 for _, h in ref)          # a fired window without a hit
    hit_edges = 0
    for p in s.placed:
        if p.kind in ("end", "start") and p.window:
            h = dict(ref)[p.window]
            lo = np.searchsorted(s.ts, p.window[0])
            hit_edges += int(np.any(s.ts[lo + h] == p.ts))
    assert hit_edges >= 1


@pytest.mark.parametrize("size,slide", SC.CUT_GEOMETRIES)
def test_cut_and_gap_builders(oracle_mod, size, slide):
    s = SC.case_stream(oracle_mod, (size, slide, "negative", SC.CUT_K))
    n = len(s.ts)
    st = set(SC.pane_starts(s).tolist())
    for name, f in SC.CUTS.items():
        c = f(s)
        assert c[0] == 0 and c[-1] == n and all(a < b for a, b in zip(c[:-1], c[1:])), name
    assert len(SC.cut_whole(s)) == 2
    assert len(SC.cut_on_panes(s)) > 5 and set(SC.cut_on_panes(s)[1:-1]) <= st
    assert SC.max_batches_per_pane(s, SC.cut_mid(s)) >= 3
    c = SC.cut_singles(s)
    ones = [a for a, b in zip(c[:-1], c[1:]) if b - a == 1]
    assert len(ones) >= 45 and any(a in st for a in ones[1:])   # the run crosses a pane's first point
    assert SC.slice_parities(s, SC.cut_odd_even(s)) == {0, 1}
    fired = set(SC.expected_windows(s.ts, size, slide))
    for kind in ("bridge", "exact", "ring"):
        for straddle in (False, True):
            g, cuts, (first, npanes) = SC.with_gap(s, kind, straddle)
            assert npanes == SC.gap_lengths(s)[kind] and cuts[0] == 0 and cuts[-1] == len(g.ts)
            assert not np.any((g.ts >= first * s.pane) & (g.ts < (first + npanes) * s.pane))
            at = int(np.searchsorted(g.ts, first * s.pane))
            assert (at in cuts) == straddle
            lost = fired - set(SC.expected_windows(g.ts, size, slide))
            if kind == "bridge":
                assert not lost                       # every window still fires
            elif kind == "exact":
                assert lost == {(first * s.pane, first * s.pane + size)}
            else:
                assert len(lost) > (s.W + s.S + 3) // s.S
