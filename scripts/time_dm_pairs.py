#!/usr/bin/env python3
"""Cost of the rotated per-env mirror (aoenv_set_dm_pairs) on the path it runs on, and of leaving the fused step for it.
    python scripts/time_dm_pairs.py C2|C4 [n_envs] [steps] [repeats]      one line "measure() <json>"
    rocprofv3 --kernel-trace --stats -d OUT -o dmp -- python scripts/time_dm_pairs.py C2 256 64 5      per-kernel times of the same run
    cat c2.txt c4.txt | python scripts/time_dm_pairs.py --collect profiles/dm_pairs_timing.json [OUT/.../dmp_kernel_stats.csv]
C2: the bench geometry (8 m, 20 x 20 Shack-Hartmann, 256 envs, float32, photon noise, the on-device integrator); C4: the ELT geometry
(39 m, 80 x 80) with 64 envs.  States, alternating inside one process so that clock drift hits all alike:
    fused          the default path (C2: the fused step kernel), shared tables
    batched        OPT_FUSED_STEP = 0, shared tables: the kernels a rotated shard runs around its surface
    pairs_mfma     every env its own rotated mirror, k_dm_pairs_mfma
    pairs_general  the same under AOENV_PATH_DM_PAIRS_GENERAL: k_dm_pairs<float>
Each figure is ms per step of run_integrator, the median over `repeats` >= 5 timed runs of `steps` steps after a warm-up round,
torch.cuda.synchronize() on both sides.  --collect adds the derived floors of the kernel (2 R^2 A flop per env at the fp32 matrix
rate, the operand tables over the HBM rate) and, given a kernel-stats file, the two kernels' own times per launch."""
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_dm_env import GEOMETRY, run_ms  # noqa: E402  (scripts/ is the first entry of sys.path)

STATES = ("fused", "batched", "pairs_mfma", "pairs_general")
PEAK_F32_MATRIX_TFLOPS, HBM_TBPS = 157.3, 8.0                       # MI355X: fp32 matrix peak, HBM3E


def measure(which, n, steps, repeats):
    import torch
    from rlao_amd import _lib as L
    from rlao_amd.env import BatchedAOEnv
    geo = GEOMETRY[which][0]
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(geo, camera="papyrus", wfs_type="shackhartmann")
    opt = lambda k, v: L.check(env._shard.lib.aoenv_set_option(env._shard.h, k, v))
    angles = np.linspace(-3.0, 3.0, n)                              # a rotation-tolerance sweep across the shard
    t = {s: [] for s in STATES}
    fused = {}
    for rep in range(repeats + 1):
        for state in STATES:
            env.clear_dm_per_env()
            opt(L.OPT_FUSED_STEP, 0 if state == "batched" else 1)
            opt(L.OPT_FORCE_PATH, L.PATH_DM_PAIRS_GENERAL if state == "pairs_general" else 0)
            if state.startswith("pairs"):
                env.set_dm_rotation(angles)
            fused[state] = bool(env.fused_step)
            env.generate_new_phase_screen(100 + rep)
            env.dm.coefs = 0
            env.dm_prev = 0
            env.measure()
            env.reset_soft()
            ms = run_ms(env, steps)
            if rep:                                                 # (the first round is the warm-up)
                t[state].append(round(ms / steps, 6))
    out = {"geometry": which, "n_envs": n, "steps": steps, "repeats": repeats, "fused_step": fused, "R": int(env.R), "A": int(env.nValidAct),
           "ms_per_step": t, "finite": bool(torch.isfinite(env._obs).all())}
    env.close()
    print("measure() " + json.dumps(out))


def collect(path, stats=None):
    out = {"unit": "ms per step of the on-device integrator, median / min / max over the repeats of one process, the states alternating",
           "command": "python scripts/time_dm_pairs.py <geometry> | python scripts/time_dm_pairs.py --collect <file> [kernel_stats.csv]"}
    for line in sys.stdin:
        if "measure()" not in line:
            continue
        rec = json.loads(line.split("measure()", 1)[1])
        assert rec["finite"], line
        rows = {k: {"median": round(float(np.median(v)), 5), "min": round(min(v), 5), "max": round(max(v), 5), "n": len(v)}
                for k, v in rec["ms_per_step"].items()}
        res = dict({k: rec[k] for k in ("n_envs", "steps", "repeats", "fused_step", "R", "A")}, **rows)
        res["pairs_vs_batched"] = round(rows["pairs_mfma"]["median"] / rows["batched"]["median"], 4)
        res["pairs_vs_fused"] = round(rows["pairs_mfma"]["median"] / rows["fused"]["median"], 4)
        res["general_vs_mfma"] = round(rows["pairs_general"]["median"] / rows["pairs_mfma"]["median"], 4)
        R, A, n = rec["R"], rec["A"], rec["n_envs"]
        cdiv = lambda a, b: -(-a // b)
        rp, ks = cdiv(R, 128) * 128, max(8, cdiv(cdiv(A, 4), 4) * 4)   # R pad 128, ga_stride (dm_pairs.hpp)
        res["floor_us_flops"] = round(2.0 * R * R * A * n / (PEAK_F32_MATRIX_TFLOPS * 1e6), 2)
        res["floor_us_tables_hbm"] = round(2.0 * rp * 4 * ks * 4 * n / (HBM_TBPS * 1e6), 2)
        out[rec["geometry"]] = res
    if stats:
        k = {}
        with open(stats) as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                if "k_dm_pairs" in name:
                    k["k_dm_pairs_mfma" if "mfma" in name else "k_dm_pairs"] = {
                        "calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2)}
        out["kernel_us_per_launch"] = k
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--collect":
        collect(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        which = sys.argv[1] if len(sys.argv) > 1 else "C2"
        _, n0, s0 = GEOMETRY[which]
        measure(which, int(sys.argv[2]) if len(sys.argv) > 2 else n0, int(sys.argv[3]) if len(sys.argv) > 3 else s0,
                max(5, int(sys.argv[4]) if len(sys.argv) > 4 else 7))
