#!/usr/bin/env python3
"""Tuning sweep of the pipelined point kNN (the numbers behind gf_knn_plan_set_tuning's defaults):
hinted 10M-point windows at depth 3, a ring of 4 distinct windows (640 MB, beyond the Infinity
Cache), every [scan blocks, x tiles per iteration, nontemporal] variant in interleaved rounds.
Per variant and round: wall time per window over WINDOWS enqueues ending in one flush and one
synchronise, no kernel timing events in the timed region.  One JSON line per variant (min, median,
max over the rounds) in the layout of profiles/r07_knn_tuning_sweep.jsonl.

usage: python tools/knn_tuning_sweep.py OUT.jsonl [TAG]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spatialflink_amd as sf  # noqa: E402
from spatialflink_amd import _lib  # noqa: E402

B = (115.5, 117.6, 39.6, 41.1)
Q = (116.414899, 39.920374)
N = 10_000_000
WINDOWS = 400
ROUNDS = 5
VARIANTS = [(0, 2, 1)] + [(b, u, nt) for b in (768, 1024, 1280, 2048) for u in (1, 2, 4) for nt in (1, 0)]


def main():
    out = sys.argv[1]
    tag = sys.argv[2] if len(sys.argv) > 2 else "new"
    torch.cuda.set_device(0)
    wins = []
    for j in range(4):
        x, y = sf.synthetic_uniform(42 + j, N, *B)
        wins.append(sf.PointWindow.from_numpy(x, y, np.arange(N, dtype=np.int64)))
    g = sf.UniformGrid(500, *B)
    op = sf.PointPointKNNQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), g)
    q = sf.Point("q", *Q, 0, g)
    ctx, plan = op.plan(0, q, 0.5, 50)
    L = _lib.lib()
    _lib.check(L.gf_knn_plan_set_pipeline(plan, 3), ctx.handle, "pipeline")
    rec = sf.PinnedRecords(WINDOWS, 50)
    pts = [w.c_struct() for w in wins]
    refs = [C.byref(p) for p in pts]
    res = {v: [] for v in VARIANTS}
    for _ in range(ROUNDS):
        for v in VARIANTS:
            _lib.check(L.gf_knn_plan_set_tuning(plan, *v), ctx.handle, "tuning")
            for i in range(8):  # both lanes of both streams warm
                L.gf_knn_enqueue(plan, refs[i % 4], rec.ptr(i))
            L.gf_knn_plan_flush(plan)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i in range(WINDOWS):
                L.gf_knn_enqueue(plan, refs[i % 4], rec.ptr(i))
            L.gf_knn_plan_flush(plan)
            torch.cuda.synchronize()
            res[v].append((time.perf_counter() - t) / WINDOWS * 1e6)
            assert all(rec.decode(i)[0] == 0 for i in range(WINDOWS)), v
    _lib.check(L.gf_knn_plan_set_tuning(plan, 0, 2, 1), ctx.handle, "tuning")
    with open(out, "w") as f:
        for v in VARIANTS:
            r = sorted(res[v])
            line = {"tag": tag, "case": "hinted_10M_d3", "n": N, "variant": list(v), "windows": WINDOWS,
                    "us_min": round(r[0], 2), "us_med": round(statistics.median(r), 2), "us_max": round(r[-1], 2)}
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    main()
