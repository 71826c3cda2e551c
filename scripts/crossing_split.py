#!/usr/bin/env python3
"""Quiet and crossing launches of the fused step kernel, and the ring launch in front of a crossing step, from a rocprofv3 kernel
trace (`rocprofv3 --kernel-trace`, e.g. the trace pass of scripts/pmc_collect.sh).

A launch of k_env_step_sh6 that directly follows a launch of k_ring_gemm_draw_ahead -- or the classic sequence k_ring_prepare,
k_gemm_nt_mfma [, k_scatter_minmax]: the first crossing of an episode, AOENV_OPT_RING_LOOKAHEAD = 0 -- is a CROSSING step: its prologue sums the ring GEMM's slabs, scatters the ring, gathers the next
crossing's Z and rescans the screen's range.  Every other launch is a QUIET step.  Only the shard's launches count: the grid of the
step kernel is n_envs workgroups of 1024 lanes, and launches in front of the first ring launch (warm-up of the calibration shards)
are left out with --skip.
    python scripts/crossing_split.py TRACE_DIR_OR_CSV [--n-envs 256] [--skip 0] [--label NAME] [--json OUT.json]
Prints one JSON object; with --json merges it into OUT.json under the key NAME (profiles/r06_crossing_split.json).
"""
import argparse, csv, glob, json, os, statistics

RING = ("k_ring_gemm_draw_ahead",)
CLASSIC = ("k_ring_prepare", "k_scatter_minmax")
CLASSIC_GEMM = "k_gemm_nt_mfma"
STEP = "k_env_step_sh6"


def rows_of(path):
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return rows


def summary(us):
    if not us:
        return {"launches": 0}
    q = statistics.quantiles(us, n=4) if len(us) >= 4 else [min(us), statistics.median(us), max(us)]
    return {"launches": len(us), "mean_us": round(statistics.fmean(us), 3), "median_us": round(statistics.median(us), 3),
            "min_us": round(min(us), 3), "max_us": round(max(us), 3), "q1_us": round(q[0], 3), "q3_us": round(q[2], 3)}


def split(rows, n_envs, skip=0):
    quiet, crossing, ring, classic = [], [], [], []
    prev_ring = False
    seen = 0
    for r in rows:
        name = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if any(k in name for k in RING):
            ring.append(us)
            prev_ring = True
            continue
        # the classic form: k_ring_prepare, then the GEMM on its own, then (AOENV_OPT_DEFER_RING = 0) k_scatter_minmax
        if any(k in name for k in CLASSIC) or (prev_ring and CLASSIC_GEMM in name):
            classic.append(us)
            prev_ring = True
            continue
        if STEP in name and int(r["Grid_Size_X"]) == 1024 * n_envs:
            seen += 1
            if seen > skip:
                (crossing if prev_ring else quiet).append(us)
        prev_ring = False
    out = {"step_quiet": summary(quiet), "step_crossing": summary(crossing), "ring_launch": summary(ring),
           "classic_ring_kernels": summary(classic)}
    if quiet and crossing:
        out["crossing_minus_quiet_us"] = round(statistics.median(crossing) - statistics.median(quiet), 3)
        out["crossing_fraction"] = round(len(crossing) / (len(crossing) + len(quiet)), 3)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--n-envs", type=int, default=256)
    ap.add_argument("--skip", type=int, default=0)
    ap.add_argument("--label", default="trace")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = split(rows_of(a.trace), a.n_envs, a.skip)
    print(json.dumps({a.label: res}, indent=1))
    if a.json:
        doc = json.load(open(a.json)) if os.path.exists(a.json) else {}
        doc[a.label] = res
        json.dump(doc, open(a.json, "w"), indent=1)
