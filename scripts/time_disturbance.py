#!/usr/bin/env python3
"""What a command-space disturbance (BatchedAOEnv.set_disturbance) costs the on-device closed loop at the C2 geometry (8 m,
20 x 20 Shack-Hartmann, 256 envs, float32 fused step, ideal camera), one build, one session.
    python scripts/time_disturbance.py [--out file.json] [n_envs] [steps] [repeats]
(a) run_integrator with no disturbance (twice, as "a" and "a2": their difference is the A/A spread of the session);
(b) run_integrator with a two-mode, three-line disturbance, every env its own lines: the same loop plus one k_disturb_apply
    launch in front of every step.
Each figure is the median over `repeats` timed runs of `steps` steps after a warm-up round, torch.cuda.synchronize() on both
sides; the states alternate inside every round so that clock drift hits all alike.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlao_amd.env import BatchedAOEnv  # noqa: E402

GAIN = 0.5
N_MODES, N_LINES = 2, 3


def make_env(n, steps):
    geo = dict(diameter=8.0, nSubaperture=20, nPixelPerSubap=6, r0=0.13, L0=30.0, windSpeed=[10.0], windDirection=[72.0],
               fractionalR0=[1.0], altitude=[0.0], nModes=50, nLoop=steps)
    env = BatchedAOEnv(n_envs=n, device=0, dtype="f32", return_frame=False)
    env.set_params(geo, camera="ideal", wfs_type="shackhartmann", gainCL=GAIN)
    return env


def episode(env, seed):
    env.generate_new_phase_screen(seed)
    env.dm.coefs = 0
    env.dm_prev = 0
    env.measure()
    env.SR = []
    return env.reset_soft()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("n_envs", nargs="?", type=int, default=256)
    ap.add_argument("steps", nargs="?", type=int, default=512)
    ap.add_argument("repeats", nargs="?", type=int, default=9)
    a = ap.parse_args()
    n, steps, repeats = a.n_envs, a.steps, max(9, a.repeats)
    states = ("a", "b", "a2")
    envs = {k: make_env(n, steps) for k in states}
    rng = np.random.RandomState(1)
    ts = envs["b"].param.samplingTime
    envs["b"].set_disturbance(N_MODES, rng.uniform(0.2e-7, 1e-7, (n, N_MODES, N_LINES)), rng.uniform(0.01, 0.45, (n, N_MODES, N_LINES)) / ts,
                              rng.uniform(0.0, 1.0, (n, N_MODES, N_LINES)))
    t = {k: [] for k in states}
    for rep in range(repeats + 1):
        for k in states:
            episode(envs[k], 100 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            envs[k].run_integrator(0, steps, GAIN)
            torch.cuda.synchronize()
            if rep:                                                 # (the first round is the warm-up)
                t[k].append(1e3 * (time.perf_counter() - t0))
    us = {k: round(1e3 * float(np.median(v)) / steps, 3) for k, v in t.items()}
    spread = {k: [round(1e3 * min(v) / steps, 3), round(1e3 * max(v) / steps, 3)] for k, v in t.items()}
    a_a = round(abs(us["a"] - us["a2"]), 3)
    moved = float((envs["b"]._obs - envs["a"]._obs).abs().max())      # same screens, same loop: the disturbance alone
    out = {"n_envs": n, "steps": steps, "repeats": repeats, "gain": GAIN, "n_modes": N_MODES, "n_lines": N_LINES,
           "fused_step": bool(envs["b"].fused_step),
           "us_per_step": {"run_integrator": us["a"], "run_integrator_again": us["a2"], "run_integrator_disturbed": us["b"]},
           "min_max_us_per_step": spread, "a_a_spread_us": a_a, "disturb_launch_us": round(us["b"] - 0.5 * (us["a"] + us["a2"]), 3),
           "env_steps_per_s": {k: round(n * 1e6 / v) for k, v in (("run_integrator", us["a"]), ("run_integrator_disturbed", us["b"]))},
           "max_abs_obs_difference_um": round(moved, 6),
           "finite": bool(all(torch.isfinite(e._obs).all() for e in envs.values()))}
    for e in envs.values():
        e.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
