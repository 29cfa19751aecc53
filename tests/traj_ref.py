"""Plain-Python restatement of the trajectory operators' contracts (the reference of
tests/test_traj_abi.py and tests/test_gpu_traj.py).

* group_ref: the grouping contract of gf_traj_group -- keys in first-occurrence order, segment
  offsets, window indices ascending inside each segment.
* tstats_ref: TStatsQuery.TStatsQueryWFunction.apply (TStatsQuery.java:154-188) per trajectory,
  with DistanceFunctions.java:60-63 as sqrt(dy*dy + dx*dx).  Python floats and math.sqrt are IEEE
  binary64 (no fused multiply-add), so the sums are the sequential left-to-right ones bit for bit.
* subtraj_ref: every trajectory with a flagged point, whole, as CSR.
"""
import math

import numpy as np


def group_ref(obj):
    """obj: int64 keys per point -> (keys[ntraj], seg_off[ntraj + 1], perm[n])"""
    first = {}
    segs = []
    for i, k in enumerate(np.asarray(obj, np.int64).tolist()):
        t = first.get(k)
        if t is None:
            first[k] = len(segs)
            segs.append([i])
        else:
            segs[t].append(i)
    keys = np.array(list(first.keys()), np.int64)
    off = np.zeros(len(segs) + 1, np.int64)
    if segs:
        off[1:] = np.cumsum([len(s) for s in segs])
    perm = np.array([i for s in segs for i in s], np.uint32)
    return keys, off, perm


def tstats_one(points):
    """points: iterable of (x, y, ts) in arrival order -> (S, T, speed)"""
    last, S, T = 0, 0.0, 0
    X = Y = 0.0
    for (px, py, ts) in points:
        if last == 0:  # the reference's "first point" test: lastTimestamp.equals(0L)
            last, X, Y, S, T = ts, px, py, 0.0, 0
        elif ts > last:
            S += math.sqrt((py - Y) * (py - Y) + (px - X) * (px - X))
            T += ts - last
            last, X, Y = ts, px, py
    return S, T, (S / T if T != 0 else float("nan"))  # Java 0.0 / 0 = NaN (S > 0 needs T > 0)


def tstats_ref(x, y, ts, keys, off, perm):
    """-> (keys, S float64[ntraj], T int64[ntraj], speed float64[ntraj]) in trajectory order"""
    xl, yl, tl = np.asarray(x, np.float64).tolist(), np.asarray(y, np.float64).tolist(), np.asarray(ts, np.int64).tolist()
    pl, ol = np.asarray(perm).tolist(), np.asarray(off).tolist()
    S, T, V = np.empty(len(keys), np.float64), np.empty(len(keys), np.int64), np.empty(len(keys), np.float64)
    for t in range(len(keys)):
        S[t], T[t], V[t] = tstats_one((xl[i], yl[i], tl[i]) for i in pl[ol[t]:ol[t + 1]])
    return np.asarray(keys, np.int64), S, T, V


def subtraj_ref(x, y, ts, keys, off, perm, hit):
    """hit: bool per point -> (keys[m], off[m + 1], x, y, ts, idx) of the trajectories with a hit"""
    hit = np.asarray(hit, bool)
    ok, oo, oi = [], [0], []
    for t in range(len(keys)):
        seg = perm[off[t]:off[t + 1]]
        if hit[seg].any():
            ok.append(keys[t])
            oi.append(seg)
            oo.append(oo[-1] + len(seg))
    idx = np.concatenate(oi).astype(np.uint32) if oi else np.empty(0, np.uint32)
    return (np.array(ok, np.int64), np.array(oo, np.int64), np.asarray(x)[idx], np.asarray(y)[idx],
            np.asarray(ts)[idx], idx)


def assert_stats_equal(got, exp):
    """(keys, S, T, speed) exactly; speed equal or both NaN"""
    gk, gS, gT, gV = got
    ek, eS, eT, eV = exp
    np.testing.assert_array_equal(gk, ek)
    assert gS.dtype == np.float64 and gV.dtype == np.float64
    np.testing.assert_array_equal(gS.view(np.int64), np.asarray(eS, np.float64).view(np.int64))  # bit for bit
    np.testing.assert_array_equal(gT, eT)
    np.testing.assert_array_equal(np.isnan(gV), np.isnan(eV))
    m = ~np.isnan(eV)
    np.testing.assert_array_equal(gV[m], eV[m])
