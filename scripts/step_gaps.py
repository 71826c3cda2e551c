#!/usr/bin/env python3
"""Idle time between consecutive launches of the fused step kernel, end to start, and the launches' durations by kind, from a
rocprofv3 kernel trace (`rocprofv3 --kernel-trace --output-format csv`, no counters in the run).

A gap counts where two step launches of the shard follow each other with no other kernel between them (a quiet boundary); where a
ring launch stands between them the gap is the sum of the two idle intervals around it (a crossing boundary).  Pair launches
(k_env_step_pair_sh6) and single launches are summarised apart.
    python scripts/step_gaps.py TRACE_DIR_OR_CSV [--n-envs 256] [--skip 50] [--label NAME] [--json OUT.json]
"""
import argparse, json, os, statistics
from crossing_split import rows_of, summary

STEP, PAIR = "k_env_step_sh6", "k_env_step_pair_sh6"


def gaps(rows, n_envs, skip):
    quiet_gap, cross_gap, single, pair = [], [], [], []
    prev_end, between, between_us, seen = None, 0, 0.0, 0
    for r in rows:
        name = r["Kernel_Name"]
        t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        is_step = (STEP in name or PAIR in name) and int(r["Grid_Size_X"]) == 1024 * n_envs
        if not is_step:
            between += 1
            between_us += (t1 - t0) / 1e3
            continue
        seen += 1
        if prev_end is not None and seen > skip:
            idle = (t0 - prev_end) / 1e3 - between_us
            (quiet_gap if between == 0 else cross_gap).append(idle)
            (pair if PAIR in name else single).append((t1 - t0) / 1e3)
        prev_end, between, between_us = t1, 0, 0.0
    return {"gap_quiet_boundary_us": summary(quiet_gap), "gap_crossing_boundary_us": summary(cross_gap),
            "single_launch_us": summary(single), "pair_launch_us": summary(pair)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--n-envs", type=int, default=256)
    ap.add_argument("--skip", type=int, default=50)
    ap.add_argument("--label", default="trace")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = gaps(rows_of(a.trace), a.n_envs, a.skip)
    print(json.dumps({a.label: res}, indent=1))
    if a.json:
        doc = json.load(open(a.json)) if os.path.exists(a.json) else {}
        doc[a.label] = res
        json.dump(doc, open(a.json, "w"), indent=1)
