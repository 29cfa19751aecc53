"""The flush chain of the pipelined kNN from a rocprofv3 --kernel-trace CSV: in the longest run of
back-to-back fused launches (the timed region), the time from the first launch's start to the last
launch's end, and from the last fused launch's end to the end of the last stand-alone select that
gf_knn_plan_flush puts behind it.
usage: python tools/trace_flush.py <kernel_trace.csv> [fused-name] [select-name]"""
import csv
import json
import sys


def main():
    path = sys.argv[1]
    fused = sys.argv[2] if len(sys.argv) > 2 else "knn_fused"
    select = sys.argv[3] if len(sys.argv) > 3 else "knn_select"
    f_rows, s_rows = [], []
    with open(path) as f:
        for r in csv.DictReader(f):
            t = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
            if fused in r["Kernel_Name"]:
                f_rows.append(t)
            elif select in r["Kernel_Name"]:
                s_rows.append(t)
    f_rows.sort()
    runs, cur = [], [f_rows[0]]
    for b in f_rows[1:]:
        if b[0] - max(e for _, e in cur) < 50_000:
            cur.append(b)
        else:
            runs.append(cur)
            cur = [b]
    runs.append(cur)
    run = max(runs, key=len)
    first_start = run[0][0]
    last_end = max(e for _, e in run)
    # the selects of this run's flush: those that start within 200 us of the last fused launch's end
    sel = [t for t in s_rows if run[-1][0] <= t[0] < last_end + 200_000]
    ends = sorted(e for _, e in run)
    out = {
        "launches": len(run),
        "interval_us": round((ends[-1] - ends[0]) / (len(ends) - 1) / 1e3, 3),
        "first_start_to_last_end_us": round((last_end - first_start) / 1e3, 3),
        "first_launch_us": round((run[0][1] - run[0][0]) / 1e3, 3),
        "last_launch_us": round((run[-1][1] - run[-1][0]) / 1e3, 3),
        "flush_selects": len(sel),
        "last_fused_end_to_last_select_end_us": round((max(e for _, e in sel) - last_end) / 1e3, 3) if sel else None,
        "select_us": [round((e - s) / 1e3, 3) for s, e in sel],
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
