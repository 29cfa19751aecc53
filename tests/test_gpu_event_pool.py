"""GPU: the context's two kinds of HIP event (ctx.cpp).  Timing events (KTimer) carry no system-scope
fence, ordering events (gf_ctx_join / gf_ctx_fork) no timestamp and a device-scope release; neither
is ever handed out as the other.  Checked here: kernel timing still reports positive, finite times
with an event pair around every launch, and join / fork still order work across the plan's streams
-- a record written on an auxiliary stream is complete when the context stream reads it, and a
window refilled on the context stream is complete when an auxiliary stream scans it."""
import math

import numpy as np
import pytest

from conftest import BEIJING, QPOINT

pytestmark = pytest.mark.gpu

R, K = 0.5, 50
N = 300_001


@pytest.fixture(scope="module")
def sf(gpu):
    import spatialflink_amd

    return spatialflink_amd


@pytest.fixture(scope="module")
def data(sf, oracle_mod):
    og = oracle_mod.grid(500, *BEIJING)
    out = []
    for j in range(3):
        x, y = oracle_mod.java_random_points(900 + j, N, *BEIJING)
        obj = np.arange(N, dtype=np.int64)
        ref = oracle_mod.knn(og, x, y, obj, *QPOINT, R, K)
        assert ref[0] == 0 and len(ref[1]) == K
        out.append((x, y, obj, ref))
    return out


def same(rec, ref):
    st, o, d, i = rec
    assert st == 0
    np.testing.assert_array_equal(o, ref[1])
    np.testing.assert_array_equal(d.view(np.int64), ref[2].view(np.int64))
    np.testing.assert_array_equal(i, ref[3])


def test_timing_and_stream_order_at_depth_3(sf, data):
    import torch
    from spatialflink_amd import _lib

    g = sf.UniformGrid(500, *BEIJING)
    q = sf.Point("q", *QPOINT, 0, g)
    op = sf.PointPointKNNQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), g)
    ctx, plan = op.plan(0, q, R, K)
    L = _lib.lib()
    wins = [sf.PointWindow.from_numpy(x, y, obj) for x, y, obj, _ in data]
    rb = sf.spatialOperators.knn_record_bytes(K)
    nwin = 8
    slots = torch.zeros(nwin, rb, dtype=torch.uint8, device="cuda")
    op.set_pipeline(0, q, R, K, 3)
    try:
        # an event pair around every fused launch, on both streams; two rounds, so that the second
        # draws its events from the pool the first one filled
        for rnd in range(2):
            ctx.set_timing_period(1)
            ctx.set_timing(1 << _lib.K_KNN_SCAN)
            for i in range(nwin):
                op.enqueue(wins[i % 3], q, R, K, slots[i])  # depth 3: gf_ctx_fork per enqueue
            op.flush(0, q, R, K)  # the selects still pending on either stream, then gf_ctx_join
            # the context stream (torch's) reads what the other stream's select wrote
            copy = slots.clone()
            ms, cnt = ctx.timing(_lib.K_KNN_SCAN)
            ctx.set_timing(0)
            assert cnt == nwin
            assert math.isfinite(ms) and ms > 0.0
            assert ms / cnt < 50.0, "a 300K-point scan takes microseconds"
            raw = copy.cpu().numpy()
            for i in range(nwin):
                same(sf.spatialOperators.decode_knn_record(raw[i].tobytes(), K), data[i % 3][3])
            slots.zero_()
        # fork: window 0's tensors are refilled on the context stream behind a queue of torch work;
        # the next two windows -- one per stream -- must both scan the new contents
        x2 = torch.from_numpy(data[2][0]).cuda()
        y2 = torch.from_numpy(data[2][1]).cuda()
        torch.cuda.synchronize()
        busy = torch.ones(1 << 24, device="cuda")
        for _ in range(20):
            busy.mul_(1.0001)
        wins[0].x.copy_(x2)
        wins[0].y.copy_(y2)
        _lib.check(L.gf_ctx_fork(ctx.handle), ctx.handle, "gf_ctx_fork")
        for i in range(2):
            op.enqueue(wins[0], q, R, K, slots[i])
        op.flush(0, q, R, K)
        _lib.check(L.gf_ctx_join(ctx.handle), ctx.handle, "gf_ctx_join")
        copy = slots[:2].clone()
        torch.cuda.synchronize()
        raw = copy.cpu().numpy()
        for i in range(2):
            same(sf.spatialOperators.decode_knn_record(raw[i].tobytes(), K), data[2][3])
    finally:
        ctx.set_timing(0)
        ctx.set_timing_period(1)
        op.set_pipeline(0, q, R, K, 1)
        op._plans.close()
