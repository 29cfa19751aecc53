"""The seams of the pipelined kNN enqueue path (gf_knn_enqueue at depths 2 to 4, S = depth - 1
streams, point and polygon queries): the window sizes around the scan's tail and the sample
threshold, flushes that drain a queue shorter than S, a depth change while a select is pending,
the index base carried per enqueue, the unfused k just above kFusedSelectMaxK with its
empty-queue flush, and the pane engine's merge folded into block 0 (k <= kFusedMergeMaxK) or
launched separately (above it).  Every record is compared with the oracle bit for bit.

The sampled window is kSampleMinN + 3 points (the smallest size class at which the sample kernel
runs); a 300 001-point window stands for the unsampled windows that still fill every scan block."""
import os
import re

import numpy as np
import pytest

from conftest import BEIJING, QPOINT, ROOT

pytestmark = pytest.mark.gpu

R_POINT, R_POLY, K = 0.5, 0.2, 50
# a concave shell with a hole, a few cells wide: the oracle walks the layers of every bbox cell
HOLED = [[(116.408, 39.914), (116.420, 39.915), (116.419, 39.927), (116.414, 39.922), (116.407, 39.926),
          (116.408, 39.914)],
         [(116.4115, 39.9165), (116.4145, 39.9165), (116.4145, 39.9195), (116.4115, 39.9195), (116.4115, 39.9165)]]


def header_const(name):
    text = open(os.path.join(ROOT, "spatialflink_amd", "csrc", "gf_internal.hpp")).read()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, name
    return int(eval(m.group(1), {"__builtins__": {}}))  # "256", "1 << 20"


K_FUSED_SELECT_MAX = header_const("kFusedSelectMaxK")
K_FUSED_MERGE_MAX = header_const("kFusedMergeMaxK")
SAMPLE_MIN_N = header_const("kSampleMinN")
BIG, MID = SAMPLE_MIN_N + 3, 300_001
SIZES = (BIG, MID, 0, 1, 63, 64, 65, 1001)


@pytest.fixture(scope="module")
def sf(gpu):
    import spatialflink_amd

    return spatialflink_amd


class Workload:
    """The windows (one per size, shared by every test) and the oracle's answers, computed once
    per (query kind, size, k) and never modified."""

    def __init__(self, sf, oracle_mod):
        self.sf, self.O = sf, oracle_mod
        self.grid = sf.UniformGrid(500, *BEIJING)
        self.ogrid = oracle_mod.grid(500, *BEIJING)
        self.query = {"point": sf.Point("q", *QPOINT, 0, self.grid), "poly": sf.Polygon(HOLED, self.grid)}
        self.opoly = oracle_mod.Polygons([self.query["poly"].rings])
        self.r = {"point": R_POINT, "poly": R_POLY}
        self.win = {}
        for n in SIZES:
            x, y = oracle_mod.java_random_points(100 + n % 97, n, *BEIJING)
            obj = (np.random.default_rng(n).permutation(n) % max(1, n // 2)).astype(np.int64)  # duplicates
            self.win[n] = (x, y, obj, sf.PointWindow.from_numpy(x, y, obj))
        self._exp = {}

    def op(self, kind):
        conf = self.sf.QueryConfiguration(self.sf.QueryType.WindowBased)
        cls = self.sf.PointPointKNNQuery if kind == "point" else self.sf.PointPolygonKNNQuery
        return cls(conf, self.grid)

    def expected(self, kind, n, k):
        key = (kind, n, k)
        if key not in self._exp:
            x, y, obj, _ = self.win[n]
            if kind == "point":
                st, o, d, i = self.O.knn(self.ogrid, x, y, obj, QPOINT[0], QPOINT[1], R_POINT, k)
                assert st == 0
            else:
                _, o, d, i = self.O.knn_ppoly(self.ogrid, x, y, obj, self.opoly, R_POLY, k)
            for a in (o, d, i):
                a.setflags(write=False)
            self._exp[key] = (o, d, i)
        return self._exp[key]


@pytest.fixture(scope="module")
def wl(sf, oracle_mod):
    return Workload(sf, oracle_mod)


class Plan:
    """One plan driven through enqueue / flush / set_pipeline, its records in pinned memory."""

    def __init__(self, wl, kind, k, slots=64):
        self.wl, self.kind, self.k = wl, kind, k
        self.op = wl.op(kind)
        self.q, self.r = wl.query[kind], wl.r[kind]
        self.rec = wl.sf.PinnedRecords(slots, k)
        self.sent = []  # (window size, index base) per record
        self.final = 0  # records checked that were final as written (no re-evaluation)

    def close(self):
        """Release the plans and the pinned records now, not at interpreter exit."""
        self.op._plans.close()
        self.rec.__del__()

    def handle(self):
        return self.op.plan(0, self.q, self.r, self.k)[1]

    def depth(self, d):
        self.op.set_pipeline(0, self.q, self.r, self.k, d)

    def index_base(self, base):
        from spatialflink_amd import _lib

        assert _lib.lib().gf_knn_plan_set_index_base(self.handle(), int(base)) == 0

    def enqueue(self, n, base=0):
        assert len(self.sent) < self.rec.count
        self.op.enqueue(self.wl.win[n][3], self.q, self.r, self.k, self.rec.ptr(len(self.sent)))
        self.sent.append((n, base))

    def flush(self):
        self.op.flush(0, self.q, self.r, self.k)

    def check(self, first=0):
        """Records first.. against the oracle (after a flush); returns them decoded.  A final
        record (status 0) is compared as the device wrote it; a flagged one (a lane's hint from a
        denser window left fewer than k below the threshold) is re-evaluated exactly by finish(),
        which applies the plan's index base of that moment -- set to the record's own."""
        import torch

        torch.cuda.synchronize()
        out = []
        for i in range(first, len(self.sent)):
            n, base = self.sent[i]
            status = self.rec.decode(i)[0]
            self.final += status == 0
            if status != 0:
                self.index_base(base)
            res = self.op.finish(self.wl.win[n][3], self.q, self.r, self.k, self.rec.raw(i))
            eo, ed, ei = self.wl.expected(self.kind, n, self.k)
            msg = f"record {i}: window of {n} points"
            np.testing.assert_array_equal(res.objID, eo, err_msg=msg)
            np.testing.assert_array_equal(res.dist.view(np.int64), ed.view(np.int64), err_msg=msg)
            np.testing.assert_array_equal(res.idx, ei + base, err_msg=msg)
            out.append(res)
        return out


@pytest.fixture
def plan(wl):
    """Plan factory; whatever a test made is released at its teardown, passed or failed."""
    made = []

    def make(kind, k):
        made.append(Plan(wl, kind, k))
        return made[-1]

    yield make
    for p in made:
        p.close()


KINDS = ("point", "poly")


@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_window_sizes(wl, plan, kind, depth):
    """A sampled window, then the empty window, one point, the sizes around one wave, an odd last
    point, the unsampled 300 001, and the sampled window again on warm lanes."""
    p = plan(kind, K)
    p.depth(depth)
    for n in (BIG, 0, 1, 63, 64, 65, 1001, MID, BIG, 1001, BIG):
        p.enqueue(n)
    p.flush()
    p.check()
    p.depth(1)


@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_flush_and_depth_changes(wl, plan, kind, depth):
    """2S + 1 windows, flush, S - 1 more, flush (a queue shorter than S); one window pending
    across set_pipeline to another depth; then down to depth 1 on the same plan, where every
    window is evaluated once more: all records equal the oracle's and the depth-1 ones."""
    small = (1001, 65, MID, 64, 63, 1, 0)
    p = plan(kind, K)
    S = depth - 1
    p.depth(depth)
    for i in range(2 * S + 1):
        p.enqueue(small[i % len(small)])
    p.flush()
    done = len(p.sent)
    got = p.check()
    for i in range(S - 1):
        p.enqueue(small[(i + 3) % len(small)])
    p.flush()
    got += p.check(done)
    p.enqueue(1001)  # pending while the depth changes
    done = len(p.sent) - 1
    other = depth + 1 if depth < 4 else 2
    for d in range(other, 0, -1):
        p.depth(d)  # completes what is pending
        got += p.check(done)
        done = len(p.sent)
        for i in range(3 if d > 1 else 0):
            p.enqueue(small[(i + d) % len(small)])
    assert done == len(p.sent)
    first = {}  # depth 1, same plan: one record per window size
    for n in small:
        first[n] = len(p.sent)
        p.enqueue(n)
    p.flush()
    ref = p.check(done)
    assert len(got) == done
    for i, res in enumerate(got):
        one = ref[first[p.sent[i][0]] - done]
        np.testing.assert_array_equal(res.objID, one.objID)
        np.testing.assert_array_equal(res.dist.view(np.int64), one.dist.view(np.int64))
        np.testing.assert_array_equal(res.idx, one.idx)


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_index_base_per_enqueue(wl, plan, kind, depth):
    """The index base changes between consecutive enqueues (the pane engine does this at depth 2):
    a record carries the base in force at its own enqueue, not at the launch that selects it."""
    p = plan(kind, K)
    p.depth(depth)
    seq = ((1001, 0), (1001, 1001), (1001, 7), (1001, 1 << 33), (1001, 5), (1001, 123_456_789), (1001, 42),
           (1001, 4242), (MID, 99_991), (65, 31), (1001, 77))
    for n, base in seq:
        p.index_base(base)
        p.enqueue(n, base)
    p.index_base(99)  # after the last enqueue: no record carries it
    p.flush()
    p.check()
    # the repeated window keeps every lane's hint valid, so those records were final as written
    assert p.final >= 9, p.final
    p.index_base(0)
    p.depth(1)


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_mid_range_k_unfused(wl, plan, kind, depth):
    """k one above kFusedSelectMaxK: [sample] + scan + select per window on S streams, nothing
    left pending, so the flush finds an empty queue (and joins the other streams at S > 1)."""
    p = plan(kind, K_FUSED_SELECT_MAX + 1)
    p.depth(depth)
    for n in (BIG, 1001, MID, 0, 65, BIG, 63):
        p.enqueue(n)
    p.flush()
    p.check()
    p.flush()  # idle plan
    p.depth(1)


@pytest.mark.parametrize("k", [K_FUSED_MERGE_MAX, K_FUSED_MERGE_MAX + 1])
def test_sliding_merge_folded_and_separate(wl, sf, oracle_mod, k):
    """Depth-2 pane engine over small panes with an empty pane between two non-empty ones (the
    engine flushes the plan while a select is pending): the window merge rides block 0 of the
    next fused launch for k <= kFusedMergeMaxK and is its own launch just above."""
    conf = sf.QueryConfiguration(sf.QueryType.WindowBased)
    op = sf.SlidingKNNQuery(conf, wl.grid, wl.query["point"], R_POINT, k, size_ms=3000, slide_ms=1000, pipeline=2)
    sizes = {10: 1001, 11: 65, 13: 64, 14: 1001, 15: 63, 17: 1}  # panes 12 and 16 are empty
    for pane, n in sizes.items():
        op.push_pane(pane, wl.win[n][3])
    op.flush()
    try:
        got = op.results()
    finally:
        op.close()
    windows = [e for e in range(10, 17 + 3) if any(q in sizes for q in range(e - 2, e + 1))]
    assert [(r.windowStart, r.windowEnd) for r in got] == [((e - 2) * 1000, (e + 1) * 1000) for e in windows]
    for r, e in zip(got, windows):
        parts = [wl.win[sizes[q]] for q in range(e - 2, e + 1) if q in sizes]
        x, y, obj = (np.concatenate([p[c] for p in parts]) for c in range(3))
        st, eo, ed, ei = oracle_mod.knn(wl.ogrid, x, y, obj, QPOINT[0], QPOINT[1], R_POINT, k)
        assert st == 0
        np.testing.assert_array_equal(r.objID, eo)
        np.testing.assert_array_equal(r.dist.view(np.int64), ed.view(np.int64))
        np.testing.assert_array_equal(r.idx, ei)
